"""kasportsformer_amd.AdamW and its two kernels on the device (include/kasf.h: kasf_adamw_segments, kasf_grad_norm; csrc/k_optim.hip): the kernels through the
C-ABI on the odd layout of tests/optim_ref.py, bit for bit; the optimiser against FusedAdamW (bits) and against a stock torch.optim.AdamW fed the same gradients
(1e-6, the bar tests/test_gpu_ops.py::test_loss3_and_adamw holds kasf_adamw_step to at this learning rate): groups, subsets, grad-is-None, per-parameter steps,
norm clipping, state interchange, checkpoints, the training loop and the wrappers.  Model: n_layers=1, n_frames=9, two clips."""
import copy

import numpy as np
import pytest
import torch

from oracle import kasf_oracle as O
from tests import optim_ref as R
from tests.gpu_util import stream
from tests.optim_ref import F32, Guarded, bits

pytestmark = pytest.mark.gpu
T, B, BAR = 9, 2, 1e-6
LR, WD = 5e-4, 0.01


@pytest.fixture(scope="module")
def seeded():
    """Name-seeded, non-identity parameters, computed once and never changed."""
    return O.name_seeded_fill(O.KASportsFormerOracle(n_layers=1, num_heads=8, n_frames=T).state_dict())


def make_model(seeded, cd="fp32"):
    import kasportsformer_amd as K
    m = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=T, compute_dtype=cd)
    m.load_state_dict(seeded, strict=True)
    return m.cuda().train()


def backward(model, opt, seed, scale=1.0, return_rep=False):
    """forward, zero_grad, loss, backward -- the loop's order; the loss scaled by `scale`."""
    import kasportsformer_amd as K
    x, y = (t.cuda() for t in O.synthetic_clips(B, T, seed=seed))
    out = model(x, return_rep=return_rep)
    opt.zero_grad()
    loss = out.square().mean() if return_rep else K.loss3(out, y)[0]
    (loss * scale).backward()


class Mirror:
    """A stock torch.optim.AdamW over plain copies of the parameters, same groups, fed the SAME gradients: p.grad is copied across before every step."""

    def __init__(self, opt, clip=None):
        self.src = [p for g in opt.param_groups for p in g["params"]]
        self.copy = [p.detach().clone().requires_grad_() for p in self.src]
        it = iter(self.copy)
        groups = [{**{k: v for k, v in g.items() if k in ("lr", "betas", "eps", "weight_decay")}, "params": [next(it) for _ in g["params"]]}
                  for g in opt.param_groups]
        self.opt, self.clip = torch.optim.AdamW(groups), clip

    def step(self):
        for p, q in zip(self.src, self.copy):
            q.grad = None if p.grad is None else p.grad.detach().clone()
        if self.clip is not None:
            torch.nn.utils.clip_grad_norm_([q for q in self.copy if q.grad is not None], self.clip)
        self.opt.step()

    def max_diff(self):
        return max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(self.src, self.copy))


def device_arrays(arrs):
    """p, g, m, v on the device behind canaries, 16-byte aligned like their host images."""
    guards = [Guarded(a) for a in arrs]
    bufs = [torch.from_numpy(q.buf.copy()).cuda() for q in guards]
    views = [b[q.start:q.start + len(q.data)] for b, q in zip(bufs, guards)]
    assert all(v.data_ptr() % 16 == 0 for v in views)
    return guards, bufs, views


def class_array(classes):
    from kasportsformer_amd import _lib
    arr = (_lib.KasfAdamwClass * len(classes))()
    for k, (lr, b1, b2, eps, wd, step) in enumerate(classes):
        arr[k] = _lib.KasfAdamwClass(lr, b1, b2, eps, wd, 0.0, 0.0, step)
    return arr


# ---------------------------------------------------------------------------------------------------------------- 1. the kernels through the C-ABI
def test_kernels_on_the_odd_layout_bit_for_bit():
    from kasportsformer_amd import _lib
    from kasportsformer_amd.optim import plan_chunks
    lib = _lib.load()
    arrs, mask = R.payloads(11), R.listed_mask()
    tbl = plan_chunks(*zip(*R.SEGMENTS))
    d_tbl = torch.from_numpy(tbl.view(np.int64).reshape(-1, 2).copy()).cuda()
    gs = 0.37
    # the norm first: value, bits from run to run, special values
    g_dev = torch.from_numpy(arrs[1]).cuda()
    partial, out2 = torch.empty(len(tbl), dtype=torch.float64, device="cuda"), torch.full((2,), -7.0, device="cuda")
    def norm(g, max_norm):
        _lib.check(lib.kasf_grad_norm(g.data_ptr(), R.N_FLAT, d_tbl.data_ptr(), len(tbl), partial.data_ptr(), gs, max_norm, out2.data_ptr(), stream()))
        return out2.cpu().numpy().copy()
    first = norm(g_dev, 1.0)
    want = R.norm_ref(arrs[1], mask, gs)
    rel = abs(float(first[0]) - want) / want
    print(f"norm {first[0]!r} against {want!r}: relative error {rel:.3e} (bound {2.0 ** -22:.3e})")
    assert rel <= 2.0 ** -22 and first[1] == min(F32(1.0), F32(1.0) / (first[0] + F32(1e-6)))
    assert np.array_equal(bits(norm(g_dev, 1.0)), bits(first))
    assert bits(norm(g_dev, float("inf")))[1] == bits(F32(1.0))
    for bad, check in ((np.inf, lambda o: np.isposinf(o[0]) and o[1] == 0.0), (np.nan, lambda o: np.isnan(o[0]) and np.isnan(o[1]))):
        gb = arrs[1].copy(); gb[4171] = bad
        assert check(norm(torch.from_numpy(gb).cuda(), 1.0)), bad
    clip = torch.tensor(norm(g_dev, 10.0), device="cuda")
    assert 0.0 < float(clip[1]) < 1.0
    # the update: without clip, with a coefficient of exactly one (same bits), with a real one
    for clip_dev, s in ((None, F32(gs)), (torch.tensor([9.0, 1.0], device="cuda"), F32(gs)), (clip, F32(gs) * F32(clip[1].item()))):
        guards, bufs, views = device_arrays(arrs)
        _lib.check(lib.kasf_adamw_segments(*(v.data_ptr() for v in views), R.N_FLAT, d_tbl.data_ptr(), len(tbl), class_array(R.CLASSES), len(R.CLASSES), gs,
                                           None if clip_dev is None else clip_dev.data_ptr(), stream()))
        want = R.expected(arrs, s)
        for name, q, b, w, before in zip("pgmv", guards, bufs, want, arrs):
            q.buf[:] = b.cpu().numpy()
            assert q.canaries_intact(), name
            assert np.array_equal(bits(q.data)[~mask], bits(before)[~mask]), f"{name}: an element outside the listed ones changed"
            assert np.array_equal(bits(q.data)[mask], bits(w)[mask]), f"{name}: listed elements differ from the restatement"
    # n_chunks == 0 touches nothing; the argument checks
    guards, bufs, views = device_arrays(arrs)
    _lib.check(lib.kasf_adamw_segments(*(v.data_ptr() for v in views), R.N_FLAT, None, 0, class_array(R.CLASSES), 2, gs, None, stream()))
    assert all(np.array_equal(b.cpu().numpy().view(np.uint32), q.buf.view(np.uint32)) for b, q in zip(bufs, guards))
    ptrs = [v.data_ptr() for v in views]
    assert lib.kasf_adamw_segments(*ptrs, R.N_FLAT, d_tbl.data_ptr(), len(tbl), class_array(R.CLASSES), 33, gs, None, stream()) == 2
    assert lib.kasf_adamw_segments(*ptrs, R.N_FLAT, d_tbl.data_ptr(), len(tbl), class_array(R.CLASSES), 0, gs, None, stream()) == 2
    assert lib.kasf_adamw_segments(*ptrs, R.N_FLAT, d_tbl.data_ptr(), -1, class_array(R.CLASSES), 2, gs, None, stream()) == 2
    assert lib.kasf_adamw_segments(None, *ptrs[1:], R.N_FLAT, d_tbl.data_ptr(), len(tbl), class_array(R.CLASSES), 2, gs, None, stream()) == 2
    assert lib.kasf_grad_norm(None, R.N_FLAT, d_tbl.data_ptr(), len(tbl), partial.data_ptr(), gs, 1.0, out2.data_ptr(), stream()) == 2
    assert lib.kasf_grad_norm(g_dev.data_ptr(), R.N_FLAT, d_tbl.data_ptr(), -1, partial.data_ptr(), gs, 1.0, out2.data_ptr(), stream()) == 2


def test_one_aligned_run_has_the_bits_of_kasf_adamw_step():
    from kasportsformer_amd import _lib
    from kasportsformer_amd.optim import plan_chunks
    lib, n = _lib.load(), 3 * 4096 + 8
    arrs = [a[:n] for a in R.payloads(12)]
    tbl = plan_chunks([0], [n], [0])
    d_tbl = torch.from_numpy(tbl.view(np.int64).reshape(-1, 2).copy()).cuda()
    a, b = ([torch.from_numpy(x.copy()).cuda() for x in arrs] for _ in range(2))
    lr, b1, b2, eps, wd, step = R.CLASSES[1]
    _lib.check(lib.kasf_adamw_segments(*(t.data_ptr() for t in a), n, d_tbl.data_ptr(), len(tbl), class_array([R.CLASSES[1]]), 1, 0.5, None, stream()))
    _lib.check(lib.kasf_adamw_step(*(t.data_ptr() for t in b), n, lr, b1, b2, eps, wd, step, 0.5, stream()))
    for name, x, y, before in zip("pgmv", a, b, arrs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert not np.array_equal(a[0].cpu().numpy(), arrs[0])


# ---------------------------------------------------------------------------------------------------------------- 2. one group: FusedAdamW's bits
@pytest.mark.parametrize("cd,grad_scale", [("fp32", 1.0), ("bf16", 1.0), ("fp32", 0.5)])
def test_one_group_has_the_bits_of_fused_adamw(seeded, cd, grad_scale):
    import kasportsformer_amd as K
    ma, mb = make_model(seeded, cd), make_model(seeded, cd)
    oa, ob = K.AdamW(ma.parameters(), lr=LR, weight_decay=WD), K.FusedAdamW(mb, lr=LR, weight_decay=WD)
    oa.grad_scale = ob.grad_scale = grad_scale
    for k in range(3):
        for m, o in ((ma, oa), (mb, ob)):
            backward(m, o, 500 + k)
            o.step()
        assert torch.equal(ma._flat.view(torch.int32), mb._flat.view(torch.int32)), k
        assert torch.equal(oa._exp_avg.view(torch.int32), ob.exp_avg.view(torch.int32)) and torch.equal(oa._exp_avg_sq.view(torch.int32), ob.exp_avg_sq.view(torch.int32)), k
    assert not torch.equal(ma._flat[:ma.n_live], make_model(seeded, cd)._flat[:ma.n_live])
    assert len(oa._launches) == 1 and oa.grad_norm is None and oa.clip_coef is None


# ---------------------------------------------------------------------------------------------------------------- 3. / 4. against stock torch
def no_decay_groups(model, lr2=2e-3):
    names = {id(p): n for n, p in model.named_parameters()}
    plain = [p for p in model.parameters() if p.dim() == 1 or names[id(p)].endswith("pos_embed")]
    ids = {id(p) for p in plain}
    return [{"params": plain, "weight_decay": 0.0, "lr": lr2}, {"params": [p for p in model.parameters() if id(p) not in ids]}]


@pytest.mark.parametrize("groups", ["one", "no_decay"])
def test_against_stock_adamw_fed_the_same_gradients(seeded, groups):
    import kasportsformer_amd as K
    model = make_model(seeded)
    opt = K.AdamW(model.parameters() if groups == "one" else no_decay_groups(model), lr=LR, weight_decay=WD)
    ref = Mirror(opt)
    if groups == "no_decay":
        assert len(opt.param_groups[0]["params"]) > 100 and any(p.dim() == 3 for p in opt.param_groups[0]["params"])
    for k in range(3):
        backward(model, opt, 520 + k)
        ref.step()
        opt.step()
        d = ref.max_diff()
        print(f"{groups} step {k}: max |dp| against stock torch {d:.3e}")
        assert d < BAR, k
    assert len(opt._launches) == 1, "all groups in one launch"
    assert float((model.head.weight.detach() - make_model(seeded).head.weight.detach()).abs().max()) > 1e-4


def test_head_only_leaves_every_other_parameter_alone(seeded):
    import kasportsformer_amd as K
    model = make_model(seeded)
    for n, p in model.named_parameters():
        if not n.startswith("head."):
            p.requires_grad_(False)
    model.pos_embed.requires_grad_(True)          # the model's switch for forming parameter gradients at all (model.forward): on, and kept out of the optimiser
    opt = K.AdamW(filter(lambda p: p.requires_grad and p is not model.pos_embed, model.parameters()), lr=LR, weight_decay=WD)
    assert [tuple(p.shape) for p in opt._params] == [(3, 512), (3,)]
    ref, before = Mirror(opt), model._flat.clone()
    for k in range(3):
        backward(model, opt, 530 + k)
        ref.step()
        opt.step()
    assert ref.max_diff() < BAR
    changed = (model._flat.view(torch.int32) != before.view(torch.int32)).nonzero().flatten()
    lo, hi = model._p_entries["head.weight"][0], model._p_entries["head.bias"][0] + 3
    inside = ((changed >= lo) & (changed < lo + 1536)) | ((changed >= hi - 3) & (changed < hi))
    assert len(changed) > 1000 and bool(inside.all()), "only head.weight and head.bias moved"
    assert len(opt.state) == 2


# ---------------------------------------------------------------------------------------------------------------- 5. grad is None, per-parameter steps
@pytest.fixture(scope="module")
def uneven(seeded):
    """Step 1 with return_rep=True (the head takes no part), step 2 ordinary -> (model, K.AdamW, its stock mirror), shared and left unchanged."""
    import kasportsformer_amd as K
    model = make_model(seeded)
    opt = K.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    ref = Mirror(opt)
    head0 = [model.head.weight.detach().clone(), model.head.bias.detach().clone()]
    backward(model, opt, 540, return_rep=True)
    assert model.head.weight.grad is None and model.head.bias.grad is None
    ref.step()
    opt.step()
    assert torch.equal(model.head.weight, head0[0]) and torch.equal(model.head.bias, head0[1]), "the head is bit-unchanged"
    assert model.head.weight not in opt.state and model.head.bias not in opt.state, "and has no state"
    d1 = ref.max_diff()
    backward(model, opt, 541)
    ref.step()
    opt.step()
    return model, opt, ref, d1


def test_grad_is_none_and_per_parameter_steps(uneven):
    model, opt, ref, d1 = uneven
    print(f"after the return_rep step {d1:.3e}, after the ordinary one {ref.max_diff():.3e}")
    assert d1 < BAR and ref.max_diff() < BAR
    assert len(opt._launches) == 1 and opt._launches[0][3] == 2, "two classes -- steps 1 and 2 -- in one launch"
    mine, stock = opt.state_dict()["state"], ref.opt.state_dict()["state"]
    assert sorted(mine) == sorted(stock)
    steps = {i: float(st["step"]) for i, st in mine.items()}
    assert steps == {i: float(st["step"]) for i, st in stock.items()} and set(steps.values()) == {1.0, 2.0}
    never = [i for i, p in enumerate(opt._params) if not opt._live[i]]
    assert never and all(i not in mine for i in never), "the never-used norm1_limb tensors have no state"


# ---------------------------------------------------------------------------------------------------------------- 6. clipping
SCALES = (1.0, 100.0, 0.01)


def clipped_run(seeded, max_grad_norm, mirror=False):
    import kasportsformer_amd as K
    model = make_model(seeded)
    opt = K.AdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=max_grad_norm)
    ref = Mirror(opt, clip=max_grad_norm) if mirror else None
    norms, coefs, diffs, rels = [], [], [], []
    for k, scale in enumerate(SCALES):
        backward(model, opt, 560 + k, scale=scale)
        kept = [None if p.grad is None else p.grad.clone() for p in opt._params]
        if ref is not None:
            want = float(torch.sqrt(sum((g.double() ** 2).sum() for g in kept if g is not None)))
            ref.step()
        opt.step()
        assert all((a is None and p.grad is None) or torch.equal(a, p.grad) for a, p in zip(kept, opt._params)), "p.grad is unchanged by step()"
        if max_grad_norm is not None:
            norms.append(opt.grad_norm.clone()); coefs.append(opt.clip_coef.clone())
        if ref is not None:
            diffs.append(ref.max_diff()); rels.append(abs(float(opt.grad_norm) - want) / want)
    return model, norms, coefs, diffs, rels


def test_norm_clipping(seeded):
    model, norms, coefs, diffs, rels = clipped_run(seeded, 1.0, mirror=True)
    plain = clipped_run(seeded, None)[0]
    gap = float((model._flat - plain._flat).abs().max())
    print(f"norms {[float(n) for n in norms]} coefficients {[float(c) for c in coefs]}; clipped against unclipped {gap:.3e}; "
          f"against clip_grad_norm_ + stock AdamW per step {diffs}; grad_norm relative error {rels} (bound {2.0 ** -22:.3e})")
    assert gap > 1e-4, "the comparison shows the clip, not Adam's scale invariance"
    assert len({float(c) for c in coefs}) == 3, "the coefficient differs every step"
    assert max(diffs) < BAR
    assert max(rels) <= 2.0 ** -22
    assert all(n.is_cuda and n.dim() == 0 and n.dtype == torch.float32 for n in norms + coefs)
    # 1e30 never clips: the bits of no clipping
    huge, hn, hc, _, _ = clipped_run(seeded, 1e30)
    assert torch.equal(huge._flat.view(torch.int32), plain._flat.view(torch.int32)) and all(float(c) == 1.0 for c in hc)
    # two identical runs: identical bits
    again, n2, _, _, _ = clipped_run(seeded, 1.0)
    assert torch.equal(again._flat.view(torch.int32), model._flat.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(norms, n2))


# ---------------------------------------------------------------------------------------------------------------- 7. state interchange
def test_state_interchange(seeded, uneven, tmp_path):
    import kasportsformer_amd as K
    whole, resumed = make_model(seeded), make_model(seeded)
    ow = K.AdamW(whole.parameters(), lr=LR, weight_decay=WD)
    o1 = K.AdamW(resumed.parameters(), lr=LR, weight_decay=WD)
    for k in range(3):
        backward(whole, ow, 580 + k)
        ow.step()
    for k in range(2):
        backward(resumed, o1, 580 + k)
        o1.step()
    sd = o1.state_dict()
    ptrs = [t.untyped_storage().data_ptr() for st in sd["state"].values() for t in st.values()]
    assert len(set(ptrs)) == len(ptrs)
    o2 = K.AdamW(resumed.parameters(), lr=1.0, weight_decay=0.5)
    o2.load_state_dict(sd)
    # the same state into a stock AdamW over copies, one stock step on the third step's gradients
    backward(resumed, o2, 582)
    stock = Mirror(o2)
    stock.opt.load_state_dict(sd)
    stock.step()
    o2.step()
    assert torch.equal(resumed._flat.view(torch.int32), whole._flat.view(torch.int32)), "two steps, state_dict, a fresh optimiser, a third step: three uninterrupted"
    assert stock.max_diff() < BAR
    # a stock state with differing steps (the grad-is-None case's) into K.AdamW: the next step follows stock's
    _, _, uref, _ = uneven
    m3 = make_model(seeded)
    with torch.no_grad():
        for p, q in zip(m3.parameters(), uref.copy):
            p.copy_(q)
    o3 = K.AdamW(m3.parameters())
    o3.load_state_dict(uref.opt.state_dict())
    assert o3.param_groups[0]["lr"] == LR and set(o3._steps.tolist()) == {0.0, 1.0, 2.0}
    r3 = Mirror(o3)
    r3.opt.load_state_dict(copy.deepcopy(uref.opt.state_dict()))          # a stock load keeps the tensors it is given: copies, the fixture stays as it is
    backward(m3, o3, 583)
    r3.step()
    o3.step()
    assert r3.max_diff() < BAR and set(o3._steps.tolist()) == {0.0, 2.0, 3.0}
    # checkpoints: K.AdamW -> file -> K.AdamW, and a file written under FusedAdamW resumed under K.AdamW
    path = tmp_path / "ck.pt"
    K.checkpoint_save(path, 4, LR, ow, whole, 0.5, "id")
    m4 = make_model(seeded)
    o4 = K.AdamW(m4.parameters())
    info = K.checkpoint_load(path, m4, o4, resume=True)
    assert info["epoch"] == 5
    for m, o in ((whole, ow), (m4, o4)):
        backward(m, o, 584)
        o.step()
    assert torch.equal(m4._flat.view(torch.int32), whole._flat.view(torch.int32))
    mf, mk = make_model(seeded), make_model(seeded)
    of = K.FusedAdamW(mf, lr=LR, weight_decay=WD)
    for k in range(2):
        backward(mf, of, 590 + k)
        of.step()
    K.checkpoint_save(path, 0, LR, of, mf, 0.5, "id")
    ok = K.AdamW(mk.parameters())
    K.checkpoint_load(path, mk, ok, resume=True)
    for m, o in ((mf, of), (mk, ok)):
        backward(m, o, 592)
        o.step()
    assert torch.equal(mk._flat.view(torch.int32), mf._flat.view(torch.int32)), "FusedAdamW's file under K.AdamW continues with FusedAdamW's bits"
    K.checkpoint_save(path, 0, LR, ok, mk, 0.5, "id")          # and the reverse: all steps agree
    mr = make_model(seeded)
    orr = K.FusedAdamW(mr)
    K.checkpoint_load(path, mr, orr, resume=True)
    assert orr.step_index == 3 and torch.equal(orr.exp_avg, ok._exp_avg)


# ---------------------------------------------------------------------------------------------------------------- 8. the loop and the wrappers
def test_train_one_epoch_runs_with_it(seeded):
    import kasportsformer_amd as K
    model = make_model(seeded, "bf16")
    before = model._flat.clone()
    loader = [O.synthetic_clips(B, T, seed=600 + k) for k in range(2)]
    avg = K.train_one_epoch(model, loader, K.AdamW(filter(lambda p: p.requires_grad, model.parameters()), lr=LR, weight_decay=WD, max_grad_norm=1.0))
    assert set(avg) == {"loss_total", "loss_mpjpe", "loss_n_mpjpe", "loss_velocity"} and all(np.isfinite(v) for v in avg.values())
    assert not torch.equal(model._flat, before)


def test_data_parallel_at_world_size_one(seeded, tmp_path):
    import torch.distributed as dist
    import kasportsformer_amd as K
    model = make_model(seeded)
    opt = K.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    opt.grad_scale = 7.0
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        dp = K.DataParallel(model, optimizer=opt)
        assert opt.grad_scale == 1.0 and not dp._scale_in_place
        before = model._flat.clone()
        backward(model, opt, 610)
        dp.finish_gradients(opt)
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(model._flat, before)
    finally:
        model.grad_stage_hook = None
        dist.destroy_process_group()


def test_flat_gradients_only_raises_and_a_recreated_flat_array_is_followed(seeded):
    import kasportsformer_amd as K
    model = make_model(seeded)
    opt = K.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    ref = Mirror(opt)
    backward(model, opt, 620)
    ref.step()
    opt.step()
    old = model._flat
    model.to("cuda")                                # _apply re-creates the flat array; the parameters are re-pointed at the new one
    assert model._flat.data_ptr() != old.data_ptr()
    snapshot = old.clone()
    backward(model, opt, 621)
    ref.step()
    opt.step()
    assert torch.equal(old, snapshot), "the array the model left is not written any more"
    assert ref.max_diff() < BAR, "the live array is"
    model.attach_param_grads = False
    with pytest.raises(RuntimeError, match="FusedAdamW"):
        opt.step()


def test_a_gradient_the_caller_put_there_is_what_gets_applied(seeded):
    import kasportsformer_amd as K
    model = make_model(seeded)
    opt = K.AdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=1.0)
    ref = Mirror(opt, clip=1.0)
    for k in range(2):
        backward(model, opt, 640 + k)
        model.head.weight.grad = model.head.weight.grad.clone() * 3.0          # no view of the flat gradient any more
        model.norm.bias.grad = torch.full_like(model.norm.bias, 0.25)
        ref.step()
        opt.step()
        assert ref.max_diff() < BAR, k


def test_step_and_zero_grad_do_not_synchronise(seeded):
    import kasportsformer_amd as K
    model = make_model(seeded)
    opt = K.AdamW(no_decay_groups(model), lr=LR, weight_decay=WD, max_grad_norm=1.0)
    mode = torch.cuda.get_sync_debug_mode()
    try:
        for k in range(2):                         # the first step builds and uploads the table, the second reuses it
            backward(model, opt, 630 + k)
            table = opt._table
            torch.cuda.set_sync_debug_mode("error")
            with pytest.raises(RuntimeError):      # the control: a read-back does raise in this mode
                model._flat[:1].cpu()
            opt.step()
            opt.zero_grad()
            torch.cuda.set_sync_debug_mode(mode)
        assert opt._table is table, "a steady state re-plans nothing"
        sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5)
        sched.step()
        backward(model, opt, 632)
        opt.step()
        assert opt._table is table, "a learning-rate change does not rebuild the table"
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert model.flat_grad is not None
    opt.zero_grad()
    assert model.flat_grad is None and all(p.grad is None for p in model.parameters())
