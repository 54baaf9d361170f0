"""The seven-term training loss on the device (K.loss7, kasf_loss7; csrc/k_loss.hip) against the fixture the reference's own utils/loss_calc.py wrote
(tests/golden/loss7.npz): the comparisons of tests/test_loss_host_cpu.py on every shape, (300, 3) and (1, 243) included, through the Python surface and through
the C-ABI, with the project's bars for loss3 (parts 1e-5, gradient rel_err 1e-4); autograd, grad_scale, the bit contract with K.loss3, reproducibility, and
three training steps through train_one_epoch.  Each case prints its figures next to the fp32 reference's own distance from float64."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_ref
from tests.loss_ref import COLLINEAR_CLIP, TIE_CLIP, ZERO_LIMB_CLIP, case_inputs, rel_err

pytestmark = pytest.mark.gpu

FX = loss_ref.load_fixture()
RUNS = loss_ref.case_runs(FX, regular_only=True)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def cabi(pred, target, lambdas, grad_scale=1.0):
    """(losses [8 + 8 B], dpred) numpy of one kasf_loss7 call on device copies of pred / target."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    p, y = dev(pred).float().contiguous(), dev(target).float().contiguous()
    B, T = p.shape[:2]
    dpred = torch.full_like(p, float("nan"))
    losses = torch.full((8 + 8 * B,), float("nan"), device="cuda")
    lam = (C.c_float * 6)(*[float(v) for v in lambdas])
    _lib.check(lib.kasf_loss7(p.data_ptr(), y.data_ptr(), dpred.data_ptr(), losses.data_ptr(), losses.numel(), B, T, lam, grad_scale,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return losses.cpu().numpy(), dpred.cpu().numpy()


def surface(pred, target, lambdas):
    """(parts [8], pred.grad) numpy through K.loss7 and .backward()."""
    import kasportsformer_amd as K
    p = dev(pred).requires_grad_(True)
    total, parts = K.loss7(p, dev(target), *[float(v) for v in lambdas])
    assert not parts.requires_grad and parts.shape == (8,) and parts.is_cuda and total.requires_grad
    total.backward()
    assert float(total.detach()) == float(parts[0])
    return parts.cpu().numpy(), p.grad.cpu().numpy()


@pytest.mark.parametrize("case,S", RUNS)
def test_parts_and_gradient_follow_the_reference(case, S):
    pred, target = case_inputs(FX, case)
    lam = FX["lambdas_" + S]
    want, gwant = FX[f"{case}_parts64_{S}"], FX[f"{case}_grad64_{S}"]
    losses, dpred = cabi(pred, target, lam)
    parts, grad = surface(pred, target, lam)
    assert parts.tobytes() == losses[:8].tobytes() and grad.tobytes() == dpred.tobytes(), "the Python surface is the C-ABI's result"
    perr, gerr = np.abs(losses[:8].astype(np.float64) - want), rel_err(dpred, gwant)
    ref_perr, ref_gerr = np.abs(FX[f"{case}_parts32_{S}"] - want), float(FX[f"{case}_graderr32_{S}"])
    print(f"{case} {S}: parts {perr.max():.2e} ({loss_ref.NAMES[int(perr.argmax())]}; fp32 reference {ref_perr.max():.2e}), "
          f"gradient rel_err {gerr:.2e} (fp32 reference {ref_gerr:.2e})")
    assert np.isfinite(losses).all() and np.isfinite(dpred).all()
    assert perr.max() < 1e-5 and gerr < 1e-4


def test_the_special_clips():
    pred, target = case_inputs(FX, "special")
    for S in "AB":
        lam = FX["lambdas_" + S]
        losses, dpred = cabi(pred, target, lam)
        want, gwant = FX[f"special_parts64_{S}"], FX[f"special_grad64_{S}"]
        assert np.isfinite(losses).all() and np.isfinite(dpred).all()
        assert np.abs(losses[:8].astype(np.float64) - want).max() < 1e-3
        _, gvar = loss_ref.loss7_ref(pred, target, only=3)
        if lam[2] == 0:
            assert not dpred[TIE_CLIP].any()
        else:
            assert rel_err(dpred[TIE_CLIP], lam[2] * gvar[TIE_CLIP]) < 1e-4 and dpred[TIE_CLIP].any()
        print(f"special {S}: zero-length clip gradient rel_err {rel_err(dpred[ZERO_LIMB_CLIP], gwant[ZERO_LIMB_CLIP]):.2e}")
        assert rel_err(dpred[ZERO_LIMB_CLIP], gwant[ZERO_LIMB_CLIP]) < 1e-4
        assert np.isfinite(dpred[COLLINEAR_CLIP]).all()
    losses, dpred = cabi(pred[:2], target[:2], FX["lambdas_A"])
    want, gwant = loss_ref.loss7_ref(pred[:2], target[:2], FX["lambdas_A"])
    assert np.abs(losses[:8].astype(np.float64) - want).max() < 1e-5 and rel_err(dpred, gwant) < 1e-4


def test_backward_scales_with_the_incoming_gradient_and_grad_scale_is_exact():
    import kasportsformer_amd as K
    pred, target = case_inputs(FX, "r3x27")
    lam = [float(v) for v in FX["lambdas_A"]]
    _, g1 = surface(pred, target, lam)
    p = dev(pred).requires_grad_(True)
    total, _ = K.loss7(p, dev(target), *lam)
    (2 * total).backward()
    assert (p.grad.cpu().numpy() == 2 * g1).all() and g1.any()
    _, d1 = cabi(pred, target, lam)
    _, d8 = cabi(pred, target, lam, grad_scale=0.125)
    assert d1.tobytes() == g1.tobytes() and (d8 == d1 * np.float32(0.125)).all()


@pytest.mark.parametrize("case", ["r3x27", "r2x2", "r2x1", "r1x243", "r300x3", "special"])
def test_with_the_new_lambdas_zero_the_bits_are_loss3s(case):
    import kasportsformer_amd as K
    pred, target = case_inputs(FX, case)
    for lam_n, lam_v in ((0.5, 20.0), (0.25, 3.0)):
        p3, p7 = dev(pred).requires_grad_(True), dev(pred).requires_grad_(True)
        t3, parts3 = K.loss3(p3, dev(target), lam_n, lam_v)
        t7, parts7 = K.loss7(p7, dev(target), lam_n, lam_v)
        t3.backward()
        t7.backward()
        assert torch.equal(parts7[:4], parts3) and torch.equal(t3, t7) and torch.equal(p3.grad, p7.grad)
        assert bool(torch.isfinite(parts7).all())
    want = FX[f"{case}_parts64_A"]
    assert np.abs(parts7[4:].double().cpu().numpy() - want[4:]).max() < (1e-3 if case == "special" else 1e-5), "all seven parts whatever the lambdas"


def test_bits_repeat_and_a_clip_does_not_see_its_neighbours():
    a, ya = case_inputs(FX, "r3x27")
    b, yb = case_inputs(FX, "r1x81")
    lam = FX["lambdas_A"]
    pred, target = np.concatenate([a, b[:, :27]]), np.concatenate([ya, yb[:, :27]])            # four clips: dividing by 4 B is exact
    runs = [cabi(pred, target, lam) for _ in range(3)]
    for losses, dpred in runs[1:]:
        assert losses.tobytes() == runs[0][0].tobytes() and dpred.tobytes() == runs[0][1].tobytes()
    losses, dpred = runs[0]
    order = [2, 3, 0, 1]
    losses_o, dpred_o = cabi(pred[order], target[order], lam)
    assert dpred_o.tobytes() == dpred[order].tobytes(), "the same clip at another place of the batch: the same dpred rows"
    assert losses_o[8:].reshape(4, 8).tobytes() == losses[8:].reshape(4, 8)[order].tobytes()
    swapped, ys = pred.copy(), target.copy()
    swapped[1:], ys[1:] = pred[[0, 0, 0]], target[[3, 2, 1]]
    losses_s, dpred_s = cabi(swapped, ys, lam)
    assert dpred_s[0].tobytes() == dpred[0].tobytes() and losses_s[8:16].tobytes() == losses[8:16].tobytes(), "... and among other clips"
    for c in range(4):
        alone_l, alone_d = cabi(pred[c:c + 1], target[c:c + 1], lam)
        assert alone_l[8:16].tobytes() == losses[8 + 8 * c:16 + 8 * c].tobytes(), "per-clip sums of a clip alone and inside the batch"
        assert (alone_d[0] == dpred[c] * np.float32(4)).all(), "its dpred rows, up to the exact factor 4 of the batch size"


def test_cpu_tensors_raise():
    import kasportsformer_amd as K
    pred, target = (torch.as_tensor(a) for a in case_inputs(FX, "r2x2"))
    with pytest.raises(RuntimeError):
        K.loss7(pred, target, lambda_limb_len=0.5)
    with pytest.raises(RuntimeError):
        K.loss7(pred.cuda(), target, lambda_limb_len=0.5)
    with pytest.raises(ValueError):
        K.loss7(pred.cuda(), target.cuda()[:, :1], lambda_limb_len=0.5)


def test_three_training_steps_through_train_one_epoch():
    import kasportsformer_amd as K
    torch.manual_seed(0)
    model = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=27, compute_dtype="fp32").cuda()
    opt = K.FusedAdamW(model, lr=5e-4, weight_decay=0.01)
    x, y = K.synthetic_clips(2, 27)
    x, y = x.cuda(), y.cuda()
    seen = []
    hook = model.register_forward_hook(lambda m, i, o: seen.append(o.detach().double().cpu().numpy()))
    first = K.train_one_epoch(model, [(x, y)], opt, lambda_limb_len=0.5)
    rest = K.train_one_epoch(model, [(x, y), (x, y)], opt, lambda_limb_len=0.5)
    hook.remove()
    assert len(seen) == 3
    for out in (first, rest):
        assert list(out) == list(K.LOSS7_NAMES) and all(np.isfinite(v) for v in out.values())
    want, _ = loss_ref.loss7_ref(seen[0], y.cpu().numpy(), (0.5, 20.0, 0.0, 0.5, 0.0, 0.0))
    got = np.array([first[n] for n in K.LOSS7_NAMES])
    print("first step:", dict(zip(loss_ref.NAMES, np.abs(got - want))))
    assert abs(first["loss_limb_len"] - want[5]) < 1e-5
    assert np.abs(got - want).max() < 1e-5 * max(1.0, abs(want[0]))
    assert rest["loss_total"] != first["loss_total"], "the optimizer stepped"
    plain = K.train_one_epoch(model, [(x, y)], opt)
    assert list(plain) == list(K.LOSS7_NAMES[:4])
