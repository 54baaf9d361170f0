"""Host side of the seven-term training loss (kasportsformer_amd.loss7, kasf_loss7): the float64 restatement the host build and the GPU tests lean on
(tests/loss_ref.py) tied to the fixture the reference's own utils/loss_calc.py wrote (tests/golden/make_loss7_golden.py), the entry point's declaration,
export, prototype and refusals, and the Python surface."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import loss_ref
from tests.loss_ref import case_inputs, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = loss_ref.load_fixture() if os.path.exists(os.path.join(ROOT, "tests", "golden", "loss7.npz")) else None
RUNS = loss_ref.case_runs(FX, regular_only=True) if FX is not None else []


def test_fixture_loads_without_pickles_and_is_small():
    path = os.path.join(ROOT, "tests", "golden", "loss7.npz")
    assert os.path.getsize(path) < 1000 * 1000
    fx = loss_ref.load_fixture()
    assert len(RUNS) == 10 and sum(s == "B" for _, s in RUNS) == 4
    a, b = fx["lambdas_A"], fx["lambdas_B"]
    assert (a != 0).all() and (b[2:] != 0).sum() == 1 and b[3] != 0, "two nonzero sets, one with a single new lambda"
    for c in fx["cases"]:
        p, y = fx[f"{c}_pred"], fx[f"{c}_target"]
        assert p.dtype == y.dtype == np.int16 and p.shape == y.shape and p.shape[2:] == (17, 3)
        assert fx[f"{c}_grad64_A"].dtype == np.float64 and fx[f"{c}_grad64_A"].shape == p.shape and fx[f"{c}_parts64_A"].shape == (8,)


@pytest.mark.parametrize("case,S", RUNS)
def test_restatement_is_the_reference_on_the_fixture(case, S):
    pred, target = case_inputs(FX, case)
    parts, grad = loss_ref.loss7_ref(pred, target, FX["lambdas_" + S])
    assert np.abs(parts - FX[f"{case}_parts64_{S}"]).max() < 1e-12
    assert rel_err(grad, FX[f"{case}_grad64_{S}"]) < 1e-10
    # the fp32 reference's own distance from fp64, the yardstick of the kernel's margins: within what the fixture's author measured
    assert np.abs(FX[f"{case}_parts32_{S}"] - FX[f"{case}_parts64_{S}"]).max() < 1e-6 and float(FX[f"{case}_graderr32_{S}"]) < 1e-5


def test_regular_cases_stay_away_from_the_kinks():
    for case in sorted({c for c, _ in RUNS}):
        args, cosines = loss_ref.l1_arguments(*case_inputs(FX, case))
        assert args.min() >= 1e-5 and cosines.max() <= 0.999, case


def test_restatement_on_the_special_clips():
    pred, target = case_inputs(FX, "special")
    assert (pred[loss_ref.TIE_CLIP] == target[loss_ref.TIE_CLIP]).all()
    assert (pred[loss_ref.ZERO_LIMB_CLIP, :, 2] == pred[loss_ref.ZERO_LIMB_CLIP, :, 1]).all()
    p = torch.tensor(pred).double()
    cos = loss_ref.limb_cosines(p)
    assert (cos[loss_ref.COLLINEAR_CLIP, :, 3].abs() > 1 - 1e-7).all(), "angle (limb 0, limb 1) is clamped in every frame"
    theta = loss_ref.limb_angles(p)[loss_ref.ZERO_LIMB_CLIP]
    assert torch.allclose(theta[:, 3], torch.full_like(theta[:, 3], np.pi / 2)) and torch.allclose(theta[:, 4], torch.full_like(theta[:, 4], np.pi / 2))
    for S in "AB":
        parts, grad = loss_ref.loss7_ref(pred, target, FX["lambdas_" + S])
        assert np.isfinite(parts).all() and np.isfinite(grad).all()
        assert np.abs(parts - FX[f"special_parts64_{S}"]).max() < 1e-12 and rel_err(grad, FX[f"special_grad64_{S}"]) < 1e-10
    # the tie clip: nothing but the variance term has a gradient there
    _, g = loss_ref.loss7_ref(pred, target, (0.5, 20.0, 0.0, 0.3, 0.2, 0.1))
    assert not g[loss_ref.TIE_CLIP].any()
    _, g = loss_ref.loss7_ref(pred, target, FX["lambdas_A"])
    _, gvar = loss_ref.loss7_ref(pred, target, only=3)
    assert np.abs(g[loss_ref.TIE_CLIP] - FX["lambdas_A"][2] * gvar[loss_ref.TIE_CLIP]).max() < 1e-15 and g[loss_ref.TIE_CLIP].any()


def test_short_clips_have_no_temporal_terms():
    pred, target = case_inputs(FX, "r2x1")
    parts, _ = loss_ref.loss7_ref(pred, target, FX["lambdas_A"])
    assert parts[3] == 0 and parts[4] == 0 and parts[7] == 0 and parts[5] > 0 and parts[6] > 0


def test_entry_point_is_declared_exported_and_refuses_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "kasf.h")).read()
    assert "int kasf_loss7(const float* pred, const float* target, float* dpred, float* losses, int64_t losses_floats, int32_t batch, int32_t n_frames," in hdr
    assert "kasf_loss7             <-" in hdr and "utils/loss_calc.py:30-94" in hdr
    assert "kasf_loss7" in _lib.SIGNATURES and hasattr(lib, "kasf_loss7")
    assert lib.kasf_loss7.argtypes == _lib.SIGNATURES["kasf_loss7"][1] and len(lib.kasf_loss7.argtypes) == 10
    assert _lib.ABI_VERSION == lib.kasf_version() == 12
    assert f"#define KASF_LOSS7_MAX_FRAMES {_lib.LOSS7_MAX_FRAMES}" in hdr
    B, T = 2, 3
    pred, target, dpred = np.full(B * T * 51, 3, np.float32), np.full(B * T * 51, 4, np.float32), np.full(B * T * 51, 5, np.float32)
    losses = np.full(8 + 8 * B, 7, np.float32)
    lam = (C.c_float * 6)(0.5, 20.0, 0.1, 0.1, 0.1, 0.1)
    p = [a.ctypes.data_as(C.c_void_p) for a in (pred, target, dpred, losses)]

    def call(pred=p[0], target=p[1], dpred=p[2], losses=p[3], cap=8 + 8 * B, batch=B, T=T, lam=lam):
        return lib.kasf_loss7(pred, target, dpred, losses, cap, batch, T, lam, 1.0, None)

    for kw in (dict(cap=8 + 8 * B - 1), dict(cap=4 + 4 * B), dict(cap=0), dict(cap=-1)):
        assert call(**kw) == 5, kw
        assert b"8 + 8 * batch" in lib.kasf_last_error()
    for kw in (dict(batch=0), dict(batch=-1), dict(T=0), dict(T=-3), dict(T=_lib.LOSS7_MAX_FRAMES + 1), dict(pred=None), dict(target=None), dict(dpred=None),
               dict(losses=None), dict(lam=None)):
        assert call(**kw) == 2, kw
        assert lib.kasf_last_error(), kw
    assert (pred == 3).all() and (target == 4).all() and (dpred == 5).all() and (losses == 7).all(), "a refused call touches no buffer"


def test_python_surface():
    import kasportsformer_amd as K
    from kasportsformer_amd import functional
    for name in ("loss7", "LOSS7_NAMES"):
        assert name in K.__all__ and name in K.__doc__
    assert K.LOSS7_NAMES == ("loss_total", "loss_mpjpe", "loss_n_mpjpe", "loss_velocity", "loss_limb_len_var", "loss_limb_len", "loss_limb_len_cos_simi",
                             "loss_limb_len_cos_simi_velocity")
    params = inspect.signature(K.loss7).parameters
    assert list(params) == ["pred", "target", "lambda_n_mpjpe", "lambda_velocity", "lambda_limb_len_var", "lambda_limb_len", "lambda_limb_cos_simi",
                            "lambda_limb_cos_simi_velocity"]
    assert [params[n].default for n in list(params)[2:]] == [0.5, 20.0, 0.0, 0.0, 0.0, 0.0]
    assert issubclass(functional._Loss7, torch.autograd.Function)
    pred = torch.zeros(2, 3, 17, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        K.loss7(pred, torch.zeros(2, 3, 17, 3), lambda_limb_len=0.5)
    # train_one_epoch carries the four yaml names, defaulting to 0, behind the arguments it had
    params = inspect.signature(K.train_one_epoch).parameters
    assert list(params)[:7] == ["model", "train_loader", "optimizer", "data_parallel", "lambda_n_mpjpe", "lambda_mpjpe_velocity", "device"]
    for name in ("lambda_limb_len_var", "lambda_limb_len", "lambda_limb_cos_simi", "lambda_limb_cos_simi_velocity"):
        assert params[name].default == 0.0


def test_train_one_epoch_picks_the_loss_by_the_lambdas(monkeypatch):
    """All four new lambdas at 0: loss3 exactly as before (what bench.py and every older test run); any of them set: loss7 with all six."""
    from kasportsformer_amd import loop
    calls = []

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))

        def forward(self, x):
            return x * self.w

    def fake(n):
        def f(pred, y, *lambdas):
            calls.append((n, lambdas))
            return pred.sum(), torch.arange(n, dtype=torch.float32)
        return f

    monkeypatch.setattr(loop, "loss3", fake(4))
    monkeypatch.setattr(loop, "loss7", fake(8))
    model = Model()
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    data = [(torch.ones(2, 3, 17, 3), torch.zeros(2, 3, 17, 3))]
    out = loop.train_one_epoch(model, data, opt, device="cpu")
    assert calls == [(4, (0.5, 20.0))] and list(out) == list(loop.LOSS7_NAMES[:4]) and out["loss_velocity"] == 3.0
    del calls[:]
    out = loop.train_one_epoch(model, data, opt, device="cpu", lambda_n_mpjpe=0.25, lambda_limb_len=0.5)
    assert calls == [(8, (0.25, 20.0, 0.0, 0.5, 0.0, 0.0))] and list(out) == list(loop.LOSS7_NAMES) and out["loss_limb_len_cos_simi_velocity"] == 7.0
    del calls[:]
    loop.train_one_epoch(model, data, opt, device="cpu", lambda_limb_cos_simi_velocity=1e-3)
    assert calls[0][0] == 8 and calls[0][1][5] == 1e-3
