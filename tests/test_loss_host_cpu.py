"""csrc/k_loss.hip without a GPU: the kernel's own source compiled for the host with g++ (-ffp-contract=off) behind a lockstep emulation of its workgroups
(tests/host_emul/: one host thread per GPU thread, a barrier at every __syncthreads and around every shuffle) and held to the fixture the reference's own
utils/loss_calc.py wrote (tests/golden/loss7.npz), with the project's bars for loss3 (tests/test_gpu_ops.py: parts 1e-5, gradient rel_err 1e-4).  It shows the
kernel's logic, its tables and its summation orders; what only the device can show (its acosf, sqrtf and divide, the real shuffles, LDS) stays with
tests/test_gpu_loss7.py.  Every fixture shape but (300, 3): 300 workgroups of 256 host threads add nothing the others do not show.  The k_loss3 text of
csrc/k_misc.hip is cut out as it is and compiled beside it for the bit comparison of the three old terms.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import loss_ref
from tests.host_emul import CSRC, build, vp
from tests.loss_ref import COLLINEAR_CLIP, TIE_CLIP, ZERO_LIMB_CLIP, case_inputs, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def loss3_text():
    """k_loss3, k_loss3_finish and their launcher as csrc/k_misc.hip has them; only the dynamic-LDS declaration is the stand-in's."""
    src = open(os.path.join(CSRC, "k_misc.hip")).read()
    kernels = re.search(r"^__device__ __forceinline__ float norm3\(.*?(?=^// torch\.optim\.AdamW semantics)", src, re.S | re.M).group(0)
    launcher = re.search(r"^void kasf_launch_loss3\(.*?^}\n", src, re.S | re.M).group(0)
    assert kernels.count("extern __shared__ float sm[];") == 1 and "k_loss3_finish" in kernels and "k_loss3_finish" in launcher
    return kernels.replace("extern __shared__ float sm[];", "KASF_DYNAMIC_LDS(sm);") + launcher


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build(tmp_path_factory, "loss_host", "emul_loss.cpp", copy=("k_loss.hip",), generate={"k_loss3.inc": loss3_text()})


def run7(lib, pred, target, lambdas, grad_scale=1.0):
    """(launches, losses [8 + 8 B], dpred) of one emulated kasf_launch_loss7."""
    B, T = pred.shape[:2]
    pred, target = np.ascontiguousarray(pred, F32), np.ascontiguousarray(target, F32)
    dpred, losses, lam = np.full(pred.shape, np.nan, F32), np.full(8 + 8 * B, np.nan, F32), np.asarray(lambdas, F32)
    n = lib.emul_loss7(vp(pred), vp(target), vp(dpred), vp(losses), B, T, vp(lam), C.c_float(grad_scale))
    return n, losses, dpred


def run3(lib, pred, target, lam_n, lam_v):
    B, T = pred.shape[:2]
    pred, target = np.ascontiguousarray(pred, F32), np.ascontiguousarray(target, F32)
    dpred, losses = np.full(pred.shape, np.nan, F32), np.full(4 + 4 * B, np.nan, F32)
    n = lib.emul_loss3(vp(pred), vp(target), vp(dpred), vp(losses), B, T, C.c_float(lam_n), C.c_float(lam_v), C.c_float(1.0))
    return n, losses, dpred


@pytest.fixture(scope="module")
def fx():
    return loss_ref.load_fixture()


HOST_RUNS = [(c, s) for c, s in loss_ref.case_runs(loss_ref.load_fixture(), regular_only=True) if c != "r300x3"] \
    if os.path.exists(os.path.join(ROOT, "tests", "golden", "loss7.npz")) else []


def test_the_fixture_has_the_shapes_the_issue_names(fx):
    shapes = {str(c): fx[f"{c}_pred"].shape[:2] for c in fx["cases"]}
    assert shapes == {"r3x27": (3, 27), "r2x2": (2, 2), "r2x1": (2, 1), "r1x81": (1, 81), "r1x243": (1, 243), "r300x3": (300, 3), "special": (3, 9)}
    assert len(HOST_RUNS) == 9


@pytest.mark.parametrize("case,S", HOST_RUNS)
def test_kernel_source_on_the_host_follows_the_reference(case, S, emul, fx):
    pred, target = case_inputs(fx, case)
    lam = fx["lambdas_" + S]
    n, losses, dpred = run7(emul, pred, target, lam)
    assert n == 2, "one k_loss7 launch and one finish launch per call"
    want, gwant = fx[f"{case}_parts64_{S}"], fx[f"{case}_grad64_{S}"]
    perr, gerr = np.abs(losses[:8].astype(np.float64) - want).max(), rel_err(dpred, gwant)
    print(f"{case} {S}: parts {perr:.2e} (fp32 reference {np.abs(fx[f'{case}_parts32_{S}'] - want).max():.2e}), gradient rel_err {gerr:.2e} "
          f"(fp32 reference {float(fx[f'{case}_graderr32_{S}']):.2e})")
    assert np.isfinite(losses).all() and np.isfinite(dpred).all()
    assert perr < 1e-5 and gerr < 1e-4
    n2, losses2, dpred2 = run7(emul, pred, target, lam)
    assert losses2.tobytes() == losses.tobytes() and dpred2.tobytes() == dpred.tobytes(), "two runs give identical bits"


def test_per_clip_sums_add_up_to_the_parts(emul, fx):
    pred, target = case_inputs(fx, "r3x27")
    _, losses, _ = run7(emul, pred, target, fx["lambdas_A"])
    B, T = pred.shape[:2]
    sums = losses[8:].reshape(B, 8).astype(np.float64).sum(0)
    counts = np.array([B * T * 17, B * T * 17, B * (T - 1) * 17, B * 16 * (T - 1), B * T * 16, B * T * 18, B * (T - 1) * 18], np.float64)
    assert np.abs(sums[:7] / counts - losses[1:8]).max() < 1e-6 and sums[7] == 0


def test_the_special_clips(emul, fx):
    pred, target = case_inputs(fx, "special")
    for S in "AB":
        lam = fx["lambdas_" + S]
        _, losses, dpred = run7(emul, pred, target, lam)
        want, gwant = fx[f"special_parts64_{S}"], fx[f"special_grad64_{S}"]
        assert np.isfinite(losses).all() and np.isfinite(dpred).all()
        assert np.abs(losses[:8].astype(np.float64) - want).max() < 1e-3, "the collinear clip's clamped angles: parts within 1e-3"
        # the tie clip: every L1 argument and every residual is exactly 0, only the variance term has a gradient there
        _, gvar = loss_ref.loss7_ref(pred, target, only=3)
        tie = lam[2] * gvar[TIE_CLIP]
        if lam[2] == 0:
            assert not dpred[TIE_CLIP].any()
        else:
            assert rel_err(dpred[TIE_CLIP], tie) < 1e-4 and np.abs(tie).max() > 0
        # the zero-length limb: theta = pi / 2, finite, and within the bars of the regular cases
        assert rel_err(dpred[ZERO_LIMB_CLIP], gwant[ZERO_LIMB_CLIP]) < 1e-4
        assert np.isfinite(dpred[COLLINEAR_CLIP]).all()           # no comparison there: the clamp's edge
    # ... and the parts of the batch without the collinear clip meet the regular bar
    two = slice(0, 2)
    _, losses, dpred = run7(emul, pred[two], target[two], fx["lambdas_A"])
    want, gwant = loss_ref.loss7_ref(pred[two], target[two], fx["lambdas_A"])
    assert np.abs(losses[:8].astype(np.float64) - want).max() < 1e-5 and rel_err(dpred, gwant) < 1e-4


@pytest.mark.parametrize("case", ["r3x27", "r2x2", "r2x1", "r1x81", "r1x243", "special"])
def test_with_the_new_lambdas_zero_the_bits_are_loss3s(case, emul, fx):
    pred, target = case_inputs(fx, case)
    for lam_n, lam_v in ((0.5, 20.0), (0.25, 3.0)):
        n3, losses3, dpred3 = run3(emul, pred, target, lam_n, lam_v)
        n7, losses7, dpred7 = run7(emul, pred, target, (lam_n, lam_v, 0, 0, 0, 0))
        assert n3 == 2 and n7 == 2
        assert dpred7.tobytes() == dpred3.tobytes() and losses7[:4].tobytes() == losses3[:4].tobytes()
        assert np.isfinite(losses7[:8]).all(), "all seven parts are computed whatever the lambdas"
    want = fx[f"{case}_parts64_A"]
    assert np.abs(losses7[4:8].astype(np.float64) - want[4:8]).max() < (1e-3 if case == "special" else 1e-5)


def test_grad_scale_and_single_terms(emul, fx):
    pred, target = case_inputs(fx, "r2x2")
    lam = fx["lambdas_A"]
    _, _, d1 = run7(emul, pred, target, lam)
    _, _, d4 = run7(emul, pred, target, lam, grad_scale=4.0)
    assert (d4 == d1 * F32(4)).all()
    for k in range(2, 6):                      # each new term alone against the restatement's gradient of that part
        one = np.zeros(6)
        one[k] = 0.7
        _, losses, d = run7(emul, pred, target, one)
        want, gwant = loss_ref.loss7_ref(pred, target, one)
        assert np.abs(losses[:8].astype(np.float64) - want).max() < 1e-5 and rel_err(d, gwant) < 1e-4, loss_ref.NAMES[k + 1]
