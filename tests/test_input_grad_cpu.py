"""CPU-side checks of the gradient with respect to the input keypoints (include/kasf.h: kasf_op_input_grad, KASF_FLAG_INPUT_GRAD): the hand-written rule of
tests/input_grad_ref.py against torch autograd, the measurement its fp32 bar is derived from, and the C-ABI's symbol, refusals and workspace plan.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import kasf_oracle as O
from tests import input_grad_ref as G
from tests import misc_ref as R

NEW_ENTRIES = ("dx_joint3", "dbone3", "dx_input")


@pytest.fixture(scope="module")
def lib():
    from kasportsformer_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def layout(lib):
    from kasportsformer_amd import _lib
    cfg, h = _lib.KasfConfig(1, 4, 8, 4, 1, 0), C.c_void_p()
    _lib.check(lib.kasf_model_create_layout_only(C.byref(cfg), C.byref(h)))
    yield h
    lib.kasf_model_destroy(h)


@pytest.fixture(scope="module")
def params(lib, layout):
    """name -> fp32 tensor of the prologue's name-seeded parameters"""
    from kasportsformer_amd import _lib
    ents = _lib.param_entries(layout)
    return R.named(R.fill_params(ents, lib.kasf_param_count(layout)), ents, torch.float32)


@pytest.mark.parametrize("frames", G.FRAMES)
def test_the_restatement_is_autograd_of_the_prologue(frames, params):
    """fp64: d/dx of <a, x> + <b, bone_decompose(x)> + <c, refusion(x)> -- the three embeddings are Linear(3,128), so their input gradients a, b, c ARE the
    cotangents of x, bone3 and limb3 -- by torch autograd through the oracle's modules and three Linear(3,128), against the rule written out by hand.  The planted
    zero-length bones and the all-zero frame are part of every size above 2: their gradient is finite, and far from zero in the zero frame."""
    i = G.inputs(frames)
    P64 = {n: t.double() for n, t in params.items()}
    x = i["x"].double().requires_grad_()
    g = R.gen(9, frames)
    gout = [torch.randn(frames, 17, 128, generator=g, dtype=torch.float64) for _ in range(3)]
    srcs = (x, O.bone_decompose(x[None])[0], R.refusion_module(P64, torch.float64)(x[None])[0])
    total = 0
    cot = []
    for (emb, pos), src, go in zip(R.EMBED_NAMES, srcs, gout):
        lin = torch.nn.Linear(3, 128).double()
        lin.load_state_dict({"weight": P64[emb + ".weight"], "bias": P64[emb + ".bias"]})
        total = total + ((lin(src) + P64[pos][0]) * go).sum()
        cot.append(go @ P64[emb + ".weight"])            # din3 = g . W: what k_embed_bwd leaves
    total.backward()
    hand = G.input_grad_ref(x.detach(), *cot, G.limb_params(params, torch.float64))
    assert torch.isfinite(x.grad).all() and torch.isfinite(hand).all()
    err = G.frame_err(hand, x.grad)
    print(f"frames {frames}: restatement against autograd {err:.2e}")
    assert err < 1e-12
    if frames > 2:
        assert not i["x"][2].any() and float(x.grad[2].abs().max()) > 1.0, "the all-zero frame has a gradient, and not a small one"
    # each path alone is autograd of that path alone
    for k, path in enumerate(("joints", "bones", "limbs")):
        x2 = i["x"].double().requires_grad_()
        src = (x2, O.bone_decompose(x2[None])[0], R.refusion_module(P64, torch.float64)(x2[None])[0])[k]
        (src * cot[k]).sum().backward()
        alone = G.input_grad_ref(x2.detach(), *[c if j == k else None for j, c in enumerate(cot)], G.limb_params(params, torch.float64))
        assert G.frame_err(alone, x2.grad) < 1e-12, path


def test_fp32_sensitivity_is_within_the_bar(params):
    """The bar of the host and GPU tests is 8 x what a plain fp32 evaluation of the restatement loses against its fp64 evaluation at the largest shape, rounded up
    to one digit (tests/input_grad_ref.py).  Re-measured here: the fp32 evaluation itself stays within the bar, the bar lies between 8 x and 16 x the
    measurement (rounding up to one digit can at most double it), and it is far below what the whole-model tests give (1e-3)."""
    sens = G.measure_fp32_sensitivity(params)
    worst = max(sens.values())
    digit = 10.0 ** np.floor(np.log10(8 * worst))
    rounded = float(np.ceil(8 * worst / digit - 1e-9) * digit)
    print("input_grad: " + ", ".join(f"{k} {v:.2e}" for k, v in sens.items()) + f" -> 8 x {worst:.2e} = {8 * worst:.2e} -> {rounded:.0e}, bar {G.BAR32:.0e}")
    assert sens["joints"] == 0.0
    assert 0 < worst <= G.BAR32 <= 1e-3
    assert 8 * worst <= G.BAR32 <= 16 * worst, "the bar is 8 x the measured sensitivity rounded up to one digit (at most twice it): re-derive it (and DESIGN.md 7.2)"


def test_symbol_prototype_and_version(lib):
    from kasportsformer_amd import _lib
    assert "kasf_op_input_grad" in _lib.SIGNATURES and hasattr(lib, "kasf_op_input_grad")
    assert lib.kasf_op_input_grad.argtypes == _lib.SIGNATURES["kasf_op_input_grad"][1] and len(lib.kasf_op_input_grad.argtypes) == 9
    assert _lib.FLAG_INPUT_GRAD == 8
    assert _lib.ABI_VERSION == 12 and lib.kasf_version() == 12          # additive under ABI 12


def test_refusals_touch_no_device(lib, layout):
    """error 2 for a null model / params / x / dx and for frames outside [1, 2^31 / (17 * 384)), error 4 for the layout-only model: all before a device or a
    pointer is touched -- the pointers are host memory, which must come back unchanged"""
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    valid = [layout, p, p, p, p, p, p, 5, None]
    for null in (0, 1, 2, 6):
        a = list(valid)
        a[null] = None
        assert lib.kasf_op_input_grad(*a) == 2, null
        assert lib.kasf_last_error()
    big = 2 ** 31 // (17 * 384) + 1
    assert (big - 1) * 17 * 384 < 2 ** 31 <= big * 17 * 384
    for n in (0, -1, big, 2 ** 62):
        a = list(valid)
        a[7] = n
        assert lib.kasf_op_input_grad(*a) == 2, n
    for nulls in ((), (3,), (4,), (5,), (3, 4, 5)):                          # the three gradients may be absent: the arguments are then valid
        a = list(valid)
        for k in nulls:
            a[k] = None
        assert lib.kasf_op_input_grad(*a) == 4, nulls
        assert b"layout-only" in lib.kasf_last_error()
    assert not buf.any()


@pytest.mark.parametrize("flags", [1, 4], ids=["TRAIN", "KEEP"])
def test_the_flag_appends_three_entries_and_nothing_else(flags, lib):
    from kasportsformer_amd import _lib
    cfg, h = _lib.KasfConfig(2, 9, 8, 4, 1, 1), C.c_void_p()
    _lib.check(lib.kasf_model_create_layout_only(C.byref(cfg), C.byref(h)))
    try:
        B = 3
        M3 = B * 9 * 17 * 3
        for f in (flags, flags | _lib.FLAG_RETURN_REP):
            old, new = _lib.ws_entries(h, B, f), _lib.ws_entries(h, B, f | _lib.FLAG_INPUT_GRAD)
            assert not set(NEW_ENTRIES) & set(old)
            assert list(new)[:len(old)] == list(old) and tuple(list(new)[len(old):]) == NEW_ENTRIES        # dicts keep the plan's order
            assert all(new[n] == old[n] for n in old), "no existing entry moves"
            up = lambda b: (b + 255) // 256 * 256
            end = lib.kasf_workspace_bytes(h, B, f)
            for n in NEW_ENTRIES:
                assert new[n] == (end, M3, 1), n                                 # fp32 [M * 3], behind everything else
                end += up(4 * M3)
            assert lib.kasf_workspace_bytes(h, B, f | _lib.FLAG_INPUT_GRAD) == end == lib.kasf_workspace_bytes(h, B, f) + 3 * up(4 * M3)
        # a plan that keeps no activations has nowhere to put them: the flag alone changes nothing
        assert _lib.ws_entries(h, B, _lib.FLAG_INPUT_GRAD) == _lib.ws_entries(h, B, 0)
        assert lib.kasf_workspace_bytes(h, B, _lib.FLAG_INPUT_GRAD) == lib.kasf_workspace_bytes(h, B, 0)
    finally:
        lib.kasf_model_destroy(h)
