"""csrc/k_refine.hip without a GPU: the kernel's own source compiled for the host with g++ behind a lockstep emulation of a workgroup (tests/host_emul/) and held
to the numpy restatement of include/kasf.h's rule (tests/refine_ref.py) bit for bit: outputs and states, canaries around every array, inputs unchanged, rows of
no track not written, the LDS the launch asked for not overrun.  It shows the kernel's logic, its indexing and its fp32 operation order; what only the device
can show stays with tests/test_gpu_refine.py."""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build, vp
from tests.refine_ref import bundle, refine_np, same_bits, weights
from tests.smooth_ref import SHAPES
from tests.test_smooth_host_cpu import Guarded

GAPS, RADII = (0, 1, 64), (0, 1, 32)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "refine_host", "emul_refine.cpp")
    lib.emul_refine.restype = C.c_int
    return lib


def run(emul, x, off, J, Cn, score, max_gap, radius, w, with_state=True, min_score=0.3):
    N, P = x.shape[0], len(off) - 1
    out, state = Guarded(x.shape, np.float32, 9.0), Guarded((N, J), np.uint8, 77)
    keep, keep_off = x.copy(), off.copy()
    overrun = emul.emul_refine(vp(x), vp(off), C.c_int64(N), P, J, Cn, int(score), C.c_float(min_score), max_gap, radius, vp(w), vp(out.a),
                               vp(state.a) if with_state else None)
    assert overrun == 0 and out.intact() and state.intact()
    assert same_bits(x, keep) and np.array_equal(off, keep_off)
    return out.a, state.a


def expect(x, off, score, max_gap, radius, w, min_score=0.3):
    """The restatement, with what a row of no track keeps: the 9.0 / 77 the outputs were filled with."""
    want, st = refine_np(x, off, score, min_score, max_gap, w, radius)
    none = st[:, 0] == 255
    want[none], st[none] = 9.0, 77
    return want, st


@pytest.mark.parametrize("J,Cn,score", SHAPES)
@pytest.mark.parametrize("max_gap", GAPS)
@pytest.mark.parametrize("radius", RADII)
def test_kernel_source_follows_the_rule(emul, J, Cn, score, max_gap, radius):
    x, off = bundle(J, Cn, score, seed=J)
    w, _ = weights(2.0 if radius < 32 else 11.0, radius)
    want, want_state = expect(x, off, score, max_gap, radius, w)
    out, state = run(emul, x, off, J, Cn, score, max_gap, radius, w)
    assert np.array_equal(state, want_state), np.argwhere(state != want_state)[:4]
    assert same_bits(out, want), np.argwhere(out.view(np.uint32) != want.view(np.uint32))[:4]
    if max_gap == 64:
        assert all((want_state == s).any() for s in (0, 1, 2, 3))
    if max_gap == 0:
        assert not ((want_state == 1) | (want_state == 2)).any()


@pytest.mark.parametrize("J,Cn,score", SHAPES)
@pytest.mark.parametrize("offsets", ["clamped", "inner"])
def test_offsets_are_clamped_and_rows_of_no_track_not_written(emul, J, Cn, score, offsets):
    x, off = bundle(J, Cn, score, seed=3, offsets=offsets)
    w, radius = weights(2.0)
    want, want_state = expect(x, off, score, 15, radius, w)
    out, state = run(emul, x, off, J, Cn, score, 15, radius, w)
    assert np.array_equal(state, want_state) and same_bits(out, want)
    if offsets == "inner":
        assert (state[:2] == 77).all() and (state[-3:] == 77).all() and (out[:2] == 9.0).all() and (out[-3:] == 9.0).all()


@pytest.mark.parametrize("J,Cn,score", SHAPES[:2])
def test_without_a_state_output_the_rows_are_the_same(emul, J, Cn, score):
    x, off = bundle(J, Cn, score, seed=4)
    w, radius = weights(2.0)
    out, state = run(emul, x, off, J, Cn, score, 15, radius, w, with_state=False)
    assert (state == 77).all()
    assert same_bits(out, expect(x, off, score, 15, radius, w)[0])


def test_a_track_alone_equals_the_track_in_the_batch(emul):
    J, Cn, score = SHAPES[0]
    x, off = bundle(J, Cn, score, seed=6)
    w, radius = weights(2.0)
    out, state = run(emul, x, off, J, Cn, score, 15, radius, w)
    for p in (0, 7, len(off) - 2):
        lo, hi = int(off[p]), int(off[p + 1])
        if hi > lo:
            o1, s1 = run(emul, np.ascontiguousarray(x[lo:hi]), np.array([0, hi - lo], np.int64), J, Cn, score, 15, radius, w)
            assert same_bits(o1, out[lo:hi]) and np.array_equal(s1, state[lo:hi])
