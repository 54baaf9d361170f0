"""csrc/k_yuv.hip without a GPU: the kernel's own source compiled for the host with g++ behind a lockstep emulation of a workgroup (tests/host_emul/: one
host thread per GPU thread, the blocks of the grid one after the other) and held to the numpy restatement of include/kasf.h's rules
(tests/test_yuv_cpu.py, yuv_to_bgr_np), exactly.  It shows the kernel's logic and its indexing -- every plane and the output sit behind padded pitches with
canaries around the buffers and a sentinel in every row's padding, and the inputs must come back unchanged --; what only the device can show stays with
tests/test_gpu_yuv.py.

The launch chooses between the kernel's two forms by alignment (csrc/k_yuv.hip): `grid` places every base pointer on the 16-byte grid with pitches and frame
strides that are multiples of 8, which takes the vector form for the whole 2 x 8 blocks (sizes from 2 x 8 on) and quads for the remainders; `odd` places the
bases at odd addresses behind odd pitches, which takes quads for everything; `pitch` keeps the bases on the grid and makes one pitch odd."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.host_emul import PAD, SENTINEL, Plane, build, up
from tests.test_yuv_cpu import SIZES, TABLES, interleave, noise_planes, yuv_to_bgr_np

COMBOS = [(m, fr, rgb) for (m, fr) in sorted(TABLES) for rgb in (False, True)]            # the four tables, rgb off / on


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "yuv_host", "emul_yuv.cpp")
    lib.emul_yuv420_to_bgr.restype = C.c_int
    lib.emul_yuv420_to_bgr.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_int64] * 4 + [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int), C.c_int, C.c_int])
    return lib


def run(emul, y, u, v, layout, matrix="bt601", full_range=False, rgb=False, place="grid"):
    """The emulated launch on planes y [F,Hf,Wf], u, v [F,ch,cw] -> the frames [F,Hf,Wf,3]; asserts one launch, no LDS, inputs unchanged, nothing outside
    the output's payload written."""
    F, Hf, Wf = y.shape
    ch, cw = u.shape[1:]
    nv12 = layout == "nv12"
    crow = 2 * cw if nv12 else cw
    if place == "odd":
        offset, yp, cp, op = 1, Wf + 3, crow + 3, 3 * Wf + 5
        yf, cf, of = Hf * yp + 7, ch * cp + 5, Hf * op + 3
    else:
        offset, yp, cp, op = 0, up(Wf, 8) + 8, up(crow, 8) + 8, up(3 * Wf, 4) + 4
        yf, cf, of = Hf * yp + 16, ch * cp + 8, Hf * op + 12
        if place == "pitch":
            yp, yf = yp + 1, Hf * (yp + 1) + 16                # the bases stay on the grid, every second luma row does not
    ins = [Plane(F, Hf, Wf, yp, yf, offset, PAD, y)]
    if nv12:
        ins.append(Plane(F, ch, crow, cp, cf, offset, PAD, interleave(u, v)))
    else:
        ins += [Plane(F, ch, crow, cp, cf, offset, PAD, u), Plane(F, ch, crow, cp, cf, offset, PAD, v)]
    out = Plane(F, Hf, 3 * Wf, op, of, offset, SENTINEL)
    coef = (C.c_int * 5)(*TABLES[(matrix, full_range)])
    fs = (lambda s: s if F > 1 else 0)
    launches = emul.emul_yuv420_to_bgr(ins[0].ptr, ins[1].ptr, None if nv12 else ins[2].ptr, int(nv12), F, Hf, Wf, yp, cp, fs(yf), fs(cf), out.ptr, op, fs(of),
                                       coef, int(full_range), int(rgb))
    assert launches == 1, "one launch, no LDS"
    assert all(p.unchanged() for p in ins), "the planes are only read"
    assert out.only_payload_changed(), "canaries, row padding and the gaps between frames survive"
    return out.view.reshape(F, Hf, Wf, 3).copy()


def want(y, u, v, layout, **kw):
    return yuv_to_bgr_np(y, interleave(u, v), **kw) if layout == "nv12" else yuv_to_bgr_np(y, u, v, layout="i420", **kw)


@pytest.mark.parametrize("Hf,Wf", SIZES)
def test_kernel_source_equals_the_restatement(emul, Hf, Wf):
    """Every size x layout x placement x F = 1, 3; the four tables and rgb on / off rotate through the cases (all eight at every size)."""
    combos = itertools.cycle(COMBOS)
    for F in (1, 3):
        y, u, v = noise_planes(Hf, Wf, seed=1000 * Hf + Wf, frames=F)
        for layout in ("nv12", "i420"):
            for place in ("grid", "odd"):
                matrix, full_range, rgb = next(combos)
                got = run(emul, y, u, v, layout, matrix, full_range, rgb, place)
                assert np.array_equal(got, want(y, u, v, layout, matrix=matrix, full_range=full_range, rgb=rgb)), (F, layout, place, matrix, full_range, rgb)


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_every_table_and_channel_order_in_both_forms(emul, layout):
    y, u, v = noise_planes(16, 8, seed=7, frames=1)                                       # one chunk: eight blocks, or thirty-two quads
    for (matrix, full_range, rgb), place in itertools.product(COMBOS, ("grid", "odd")):
        got = run(emul, y, u, v, layout, matrix, full_range, rgb, place)
        assert np.array_equal(got, want(y, u, v, layout, matrix=matrix, full_range=full_range, rgb=rgb)), (matrix, full_range, rgb, place)
    assert np.array_equal(run(emul, y, u, v, layout, rgb=True), run(emul, y, u, v, layout)[..., ::-1])


def test_an_odd_pitch_under_aligned_bases_and_more_than_one_chunk(emul):
    y, u, v = noise_planes(37, 23, seed=3, frames=3)
    for layout in ("nv12", "i420"):
        ref = want(y, u, v, layout)
        assert np.array_equal(run(emul, y, u, v, layout, place="pitch"), ref)
        for f in range(3):                                                                # a frame alone gives what it gives in the batch
            assert np.array_equal(run(emul, y[f:f + 1], u[f:f + 1], v[f:f + 1], layout)[0], ref[f])
    y, u, v = noise_planes(40, 72, seed=9, frames=1)                                      # 180 blocks + no strip in the vector form, 720 quads = three chunks in the element form
    for layout, place in itertools.product(("nv12", "i420"), ("grid", "odd")):
        assert np.array_equal(run(emul, y, u, v, layout, place=place), want(y, u, v, layout)), (layout, place)
    y, u, v = noise_planes(45, 77, seed=11, frames=1)                                     # 198 blocks, then the right strip's and the bottom row's quads, in two chunks
    for layout in ("nv12", "i420"):
        assert np.array_equal(run(emul, y, u, v, layout), want(y, u, v, layout)), layout
