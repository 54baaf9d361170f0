"""CPU-side checks of the prologue / gate / head / embedding operator entries (include/kasf.h, kasf_op_prologue_fwd ... kasf_op_add): the symbols and prototypes,
every refusal before a device is touched, and the measurement the fp32 bars of tests/test_gpu_misc.py are derived from.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import misc_ref as R

NAMES = ("kasf_op_misc_scratch_floats", "kasf_op_prologue_fwd", "kasf_op_embed_bwd", "kasf_op_refusion_bwd", "kasf_op_gate_fwd", "kasf_op_gate_bwd",
         "kasf_op_head_fwd", "kasf_op_head_bwd", "kasf_op_rep_bwd", "kasf_op_finalize_ls", "kasf_op_add")


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


def test_symbols_and_prototypes(lib):
    from kasportsformer_amd import _lib
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]
    assert _lib.ABI_VERSION == 12 and lib.kasf_version() == 12          # additive under ABI 12


def test_scratch_sizes(lib):
    from kasportsformer_amd import _lib
    f = lib.kasf_op_misc_scratch_floats
    up = lambda v: (v + 63) // 64 * 64
    row = {_lib.MISC_EMBED_BWD: 17 * 128 + 128 * 3 + 128, _lib.MISC_GATE_BWD: 1160, _lib.MISC_HEAD_BWD: 3 * 512 + 4}
    assert f(_lib.MISC_EMBED_BWD, 1) == up(row[0]) and f(_lib.MISC_EMBED_BWD, 127) == up(127 * row[0]) and f(_lib.MISC_EMBED_BWD, 10 ** 6) == up(128 * row[0])
    assert f(_lib.MISC_GATE_BWD, 1) == up(1160) and f(_lib.MISC_GATE_BWD, 17) == up(2 * 1160) and f(_lib.MISC_GATE_BWD, 10 ** 6) == up(768 * 1160)
    assert f(_lib.MISC_HEAD_BWD, 2049) == up(129 * row[3]) and f(_lib.MISC_HEAD_BWD, 10 ** 6) == up(256 * row[3])
    # the refusion row mirrors the range of the 204 limb-MLP tensors of the flat gradient array
    assert f(_lib.MISC_REFUSION_BWD, 256) == f(_lib.MISC_REFUSION_BWD, 10 ** 6) and f(_lib.MISC_REFUSION_BWD, 256) % 64 == 0
    assert f(4, 10) == -2 and f(-1, 10) == -2 and f(0, 0) == -2 and lib.kasf_last_error()


def test_refusion_row_is_the_layouts_limb_range(lib, layout):
    from kasportsformer_amd import _lib
    ents = [(n, o, s) for n, o, s in _lib.param_entries(layout) if n.startswith("bone_refusion.")]
    assert len(ents) == 204
    lo = min(o for _, o, _ in ents)
    hi = max(o + int(np.prod(s)) for _, o, s in ents)
    assert lib.kasf_op_misc_scratch_floats(_lib.MISC_REFUSION_BWD, 1) == (hi - lo + 63) // 64 * 64


def test_refusals_touch_no_device(lib, layout):
    """every refusal is error 2 (3: dtype, 4: layout-only model) with a message, before a device or a pointer is touched: the pointers are host memory"""
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    big_frames, big_m = 2 ** 31 // (17 * 384) + 1, 2 ** 31 // 384 + 1
    assert (big_frames - 1) * 17 * 384 < 2 ** 31 <= big_frames * 17 * 384 and (big_m - 1) * 384 < 2 ** 31 <= big_m * 384

    def call(name, args, null=None, **kw):
        a = list(args)
        if null is not None:
            a[null] = None
        for k, v in kw.items():
            a[k] = v
        return getattr(lib, name)(*a)

    # name -> (valid argument list with host pointers, indices of required pointers, index of frames / M, valid return code)
    table = {
        "kasf_op_prologue_fwd": ([layout] + [p] * 7 + [5, None], range(0, 8), 8, 4),
        "kasf_op_embed_bwd": ([0] + [p] * 6 + [None, 5, None, 0, None], range(1, 7), 8, None),
        "kasf_op_refusion_bwd": ([layout] + [p] * 4 + [5, None, 0, None], range(0, 5), 5, 4),
        "kasf_op_gate_fwd": ([0] + [p] * 6 + [None, 5, 1, None], range(1, 7), 8, None),
        "kasf_op_gate_bwd": ([0, p, None, None] + [p] * 10 + [5, 1, None, 0, None], [1] + list(range(4, 14)), 14, None),
        "kasf_op_head_fwd": ([0] + [p] * 4 + [5, None], range(1, 5), 5, None),
        "kasf_op_head_bwd": ([0] + [p] * 6 + [5, None, 0, None], range(1, 7), 7, None),
        "kasf_op_rep_bwd": ([0] + [p] * 3 + [5, None], range(1, 4), 4, None),
    }
    for name, (args, ptrs, ni, valid_rc) in table.items():
        for i in ptrs:
            assert call(name, args, null=i) == 2, (name, i)
            assert lib.kasf_last_error()
        big = big_frames if name in ("kasf_op_prologue_fwd", "kasf_op_embed_bwd", "kasf_op_refusion_bwd") else big_m
        for n in (0, -1, big, 2 ** 62):
            a = list(args)
            a[ni] = n
            assert getattr(lib, name)(*a) == 2, (name, n)
        if valid_rc is not None:
            assert call(name, args) == valid_rc, name                    # the layout-only model: refused with 4, after the argument checks
            assert b"layout-only" in lib.kasf_last_error()
        if isinstance(args[0], int):
            a = list(args)
            a[0] = 2
            assert getattr(lib, name)(*a) == 3, name                      # the family's bad-dtype code
    # scratch given with no size, or misaligned
    for name in ("kasf_op_embed_bwd", "kasf_op_gate_bwd", "kasf_op_head_bwd", "kasf_op_refusion_bwd"):
        args = list(table[name][0])
        si = len(args) - 3
        args[si], args[si + 1] = p, 0
        assert getattr(lib, name)(*args) == 2, name
        args[si], args[si + 1] = C.c_void_p(p.value + 4), 1024
        assert getattr(lib, name)(*args) == 2, name
    # gate_bwd: dw / db may be absent only when adaptive == 0
    a = list(table["kasf_op_gate_bwd"][0])
    a[12] = None
    assert lib.kasf_op_gate_bwd(*a) == 2
    # finalize_ls: pointers and the two supported shapes
    fin = [p] * 6 + [128, 128, None]
    for i in range(6):
        assert call("kasf_op_finalize_ls", fin, null=i) == 2
    for N, K in ((64, 128), (128, 256), (128, 0), (0, 128), (256, 512), (128, -128)):
        a = list(fin)
        a[6], a[7] = N, K
        assert lib.kasf_op_finalize_ls(*a) == 2, (N, K)
    # add: n a multiple of 8 in [8, 2^40); c needs b
    add = [0, p, p, p, p, 64, None]
    for n in (0, -8, 7, 9, 12, 2 ** 40, 2 ** 40 + 8):
        a = list(add)
        a[5] = n
        assert lib.kasf_op_add(*a) == 2, n
    for i in (1, 2):
        assert call("kasf_op_add", add, null=i) == 2
    a = list(add)
    a[3] = None                                                           # b absent, c present
    assert lib.kasf_op_add(*a) == 2
    a = list(add)
    a[0] = 5
    assert lib.kasf_op_add(*a) == 3
    assert not buf.any()


def test_gate_backward_formula_is_autograd_of_the_forward():
    """the softmax backward written out in misc_ref.gate_bwd_ref against autograd of gate_fwd_ref: guards the reference itself"""
    i = R.gate_inputs(17)
    t = {n: v.double().requires_grad_(n in ("xa", "xg", "xb", "w", "bias")) for n, v in i.items()}
    f = R.gate_fwd_ref(t["xa"], t["xg"], t["xb"], t["w"], t["bias"], 1)
    f["out"].backward(t["g"])
    hand = R.gate_bwd_ref(t["g"], t["xa"].detach(), t["xg"].detach(), t["xb"].detach(), t["w"].detach(), f["alpha"].detach(), 1)
    for n, want in (("ga", t["xa"].grad), ("gg", t["xg"].grad), ("gb", t["xb"].grad), ("dw", t["w"].grad), ("db", t["bias"].grad)):
        assert R.rel_err(hand[n], want) < 1e-12, n


def test_fp32_sensitivity_is_within_the_bars(lib, layout):
    """The bars of tests/test_gpu_misc.py are 8 x what a plain fp32 evaluation of the reference loses against the fp64 one at each op's largest shape (DESIGN.md
    7.2).  Re-measured here: the fp32 evaluation itself must stay within every bar (no floors are used), and no bar may exceed 1e-3 (what the whole-model tests
    already give)."""
    from kasportsformer_amd import _lib
    ents = _lib.param_entries(layout)
    flat = R.fill_params(ents, lib.kasf_param_count(layout))
    P = {n: t for n, t in R.named(flat, ents, torch.float32).items() if n.split(".")[0] in ("bone_refusion", "joints_embed", "bone_embed", "limb_embed")
         or n.endswith("pos_embed")}
    sens = R.measure_fp32_sensitivity(P)
    assert set(sens) == set(R.BAR32)
    for op, d in sens.items():
        worst = max(d.values())
        print(f"{op}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()) + f" -> 8 x {worst:.2e} = {8 * worst:.2e}, bar {R.BAR32[op]:.1e}")
        assert 0 < worst <= R.BAR32[op] <= 1e-3, (op, d)
