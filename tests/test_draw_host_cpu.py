"""csrc/k_draw.hip without a GPU: the kernel's own source compiled for the host with g++ behind a lockstep emulation of a workgroup (tests/host_emul/: one
host thread per GPU thread, the blocks of the grid one after the other, __ballot modelled per wavefront of 64) and held to the numpy restatements of
include/kasf.h's rules (tests/test_draw_cpu.py: draw_poses_np, bgr_to_nv12_np, pose_panel_np), exactly.  It shows the kernel's logic -- binning, in-order
compaction, the backward walk over chunks, the per-pixel painted bits -- and its indexing: the frame, the output and both planes of the surface sit behind padded
pitches with canaries around the buffers and a sentinel in every row's padding; inputs must come back unchanged, in-place runs may change the frame's payload
only.  What only the device can show stays with tests/test_gpu_draw.py.

The launch chooses each stream's form by alignment (csrc/k_draw.hip): `grid` places every base pointer on the 16-byte grid with pitches and frame strides that
are multiples of 8, which moves whole blocks as dwords and the blocks at the frame's right and bottom edge byte by byte; `odd` places the bases at odd addresses
behind odd pitches: bytes everywhere; `pitch` keeps the bases on the grid and makes the input frame's pitch alone odd: bytes in, dwords out."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests.host_emul import PAD, SENTINEL, Plane, build, up
from tests.test_draw_cpu import CASES, COMBOS, LIST, TABLES, TILE_H, TILE_W, bgr_to_nv12_np, expected, noise_frames, pose_panel_np, primitives_through_tile

OUTPUTS = ("bgr", "surface", "both", "inplace", "inplace+surface")


class Launch(C.Structure):                                       # csrc/draw_args.h, field for field
    _fields_ = [("frames", C.c_void_p), ("n_frames", C.c_int), ("Hf", C.c_int), ("Wf", C.c_int), ("row_stride", C.c_int64), ("frame_stride", C.c_int64),
                ("keypoints", C.c_void_p), ("P", C.c_int), ("J", C.c_int), ("use_score", C.c_int), ("kp_frame_stride", C.c_int64), ("kp_person_stride", C.c_int64),
                ("kp_joint_stride", C.c_int64), ("kp_coord_stride", C.c_int64), ("valid", C.c_void_p), ("valid_frame_stride", C.c_int64),
                ("valid_person_stride", C.c_int64), ("segments", C.c_void_p), ("colors", C.c_void_p), ("S", C.c_int), ("dot_color", C.c_uint8 * 3),
                ("thickness", C.c_int), ("dot_radius", C.c_int), ("min_score", C.c_float), ("fills", C.c_void_p), ("R", C.c_int), ("out_bgr", C.c_void_p),
                ("out_row_stride", C.c_int64), ("out_frame_stride", C.c_int64), ("out_y", C.c_void_p), ("out_uv", C.c_void_p), ("y_row_stride", C.c_int64),
                ("uv_row_stride", C.c_int64), ("y_frame_stride", C.c_int64), ("uv_frame_stride", C.c_int64), ("coef", C.c_void_p), ("full_range", C.c_int),
                ("rgb", C.c_int)]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "draw_host", "emul_draw.cpp")
    lib.emul_draw_poses.restype = C.c_int
    lib.emul_draw_poses.argtypes = [C.POINTER(Launch)]
    lib.emul_pose_panel.restype = C.c_int
    lib.emul_pose_panel.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.emul_draw_constants.argtypes = [C.POINTER(C.c_int)]
    return lib


def test_the_kernels_constants_are_the_ones_the_cases_were_sized_for(emul):
    k = (C.c_int * 5)()
    emul.emul_draw_constants(k)
    assert tuple(k[:4]) == (TILE_W, TILE_H, LIST, 256) and k[4] == C.sizeof(Launch)
    case, _ = expected("chunked")
    assert primitives_through_tile(case, 0, 0) > 2 * k[2], "one tile's primitives exceed the LDS list at least twice over: the chunked path"
    Hf, Wf = expected("odd")[0]["frames"].shape[1:3]
    assert -(-Hf // k[1]) >= 3 and -(-Wf // k[0]) >= 3 and Hf % 2 and Wf % 2, "the odd frame spans 3 x 3 tiles"


def strided_copy(a, pad):
    """`a` behind padded strides in every dimension but none contiguous with the next: a view into a larger array of NaN (floats) or 0xEE (bytes)."""
    big = np.full(tuple(s + pad for s in a.shape), np.nan if a.dtype.kind == "f" else PAD, a.dtype)
    view = big[tuple(slice(1 if pad else 0, (1 if pad else 0) + s) for s in a.shape)]
    view[...] = a
    return big, view


def run(emul, case, place="grid", outputs="both", matrix="bt601", full_range=False, rgb=False):
    """The emulated launch -> (painted frames or None, y or None, uv or None); asserts one launch, inputs unchanged, nothing outside the outputs' payloads written."""
    frames, kp, valid, kw = case["frames"], case["kp"], case["valid"], case["kw"]
    F, Hf, Wf = frames.shape[:3]
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    if place == "odd":
        offset, fp, op, yp, cp = 1, 3 * Wf + 7, 3 * Wf + 5, Wf + 3, 2 * cw + 3
        ff, of, yf, cf = Hf * fp + 5, Hf * op + 3, Hf * yp + 7, ch * cp + 5
    else:
        offset, fp, op, yp, cp = 0, up(3 * Wf, 8) + 8, up(3 * Wf, 8) + 16, up(Wf, 8) + 8, up(2 * cw, 8) + 8
        ff, of, yf, cf = Hf * fp + 16, Hf * op + 24, Hf * yp + 16, ch * cp + 8
        if place == "pitch":
            fp, ff = fp + 1, Hf * (fp + 1) + 16
    src = Plane(F, Hf, 3 * Wf, fp, ff, offset, PAD, frames)
    in_place = outputs.startswith("inplace")
    out = src if in_place else (Plane(F, Hf, 3 * Wf, op, of, offset, SENTINEL) if outputs in ("bgr", "both") else None)
    want_surface = outputs in ("surface", "both", "inplace+surface")
    py = Plane(F, Hf, Wf, yp, yf, offset, SENTINEL) if want_surface else None
    puv = Plane(F, ch, 2 * cw, cp, cf, offset, SENTINEL) if want_surface else None
    fs = (lambda s: s if F > 1 else 0)
    d = Launch()
    d.frames, d.n_frames, d.Hf, d.Wf, d.row_stride, d.frame_stride = src.ptr, F, Hf, Wf, fp, fs(ff)
    keep = []
    if kp is not None and kp.shape[1] > 0:
        big, view = strided_copy(kp, 2 if place != "grid" else 0)
        keep.append((big, big.copy()))
        d.keypoints, (d.P, d.J) = view.ctypes.data, kp.shape[1:3]
        d.kp_frame_stride, d.kp_person_stride, d.kp_joint_stride, d.kp_coord_stride = (s // 4 for s in view.strides)
        d.use_score = int(kp.shape[3] == 3 and kw.get("min_score") is not None)
        if valid is not None:
            vbig, vview = strided_copy(valid.astype(np.uint8), 1 if place != "grid" else 0)
            keep.append((vbig, vbig.copy()))
            d.valid, (d.valid_frame_stride, d.valid_person_stride) = vview.ctypes.data, vview.strides
    seg, col = np.ascontiguousarray(kw["segments"], np.int32), np.ascontiguousarray(kw["colors"], np.uint8)
    fills = np.ascontiguousarray(kw["fills"], np.int32) if kw.get("fills") is not None else np.zeros((0, 7), np.int32)
    coef = np.array(TABLES[(matrix, full_range)], np.int32)
    keep += [(a, a.copy()) for a in (seg, col, fills)]
    d.segments, d.colors, d.S = seg.ctypes.data, col.ctypes.data, len(seg)
    d.dot_color = (C.c_uint8 * 3)(*kw.get("dot_color", (255, 255, 255)))
    d.thickness, d.dot_radius, d.min_score = kw.get("thickness", 2), kw.get("dot_radius", 2), kw.get("min_score") or 0.0
    d.fills, d.R = (fills.ctypes.data if len(fills) else None), len(fills)
    if out is not None:
        d.out_bgr, d.out_row_stride, d.out_frame_stride = out.ptr, out.pitch, fs(out.frame_stride)
    if want_surface:
        d.out_y, d.out_uv, d.y_row_stride, d.uv_row_stride, d.y_frame_stride, d.uv_frame_stride = py.ptr, puv.ptr, yp, cp, fs(yf), fs(cf)
    d.coef, d.full_range, d.rgb = coef.ctypes.data, int(full_range), int(rgb)
    assert emul.emul_draw_poses(C.byref(d)) == 1, "one launch"
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in keep), "keypoints, valid, segments, colours and fills are only read"
    if in_place:
        assert src.only_payload_changed(), "in place only the frame's payload changes"
    else:
        assert src.unchanged(), "the frame is only read"
    for p in (out, py, puv):
        assert p is None or p.only_payload_changed(), "canaries, row padding and the gaps between frames survive"
    return (None if out is None else out.view.reshape(F, Hf, Wf, 3).copy(), None if py is None else py.view.copy(),
            None if puv is None else puv.view.reshape(F, ch, cw, 2).copy())


@functools.lru_cache(maxsize=None)
def surface_of(name, matrix, full_range, rgb):
    return bgr_to_nv12_np(expected(name)[1], matrix, full_range, rgb)


def check(got, name, combo):
    painted, y, uv = got
    if painted is not None:
        assert np.array_equal(painted, expected(name)[1]), (name, "frame")
    if y is not None:
        wy, wuv = surface_of(name, *combo)
        assert np.array_equal(y, wy), (name, combo, "luma")
        assert np.array_equal(uv, wuv), (name, combo, "chroma")


@pytest.mark.parametrize("name", CASES)
def test_kernel_source_equals_the_restatement(emul, name):
    """Every case x placement x output set; the four tables and rgb on / off rotate through the runs."""
    case, _ = expected(name)
    combos = itertools.cycle(COMBOS)
    for place, outputs in itertools.product(("grid", "odd", "pitch"), OUTPUTS):
        combo = next(combos)
        check(run(emul, case, place, outputs, *combo), name, combo)


def test_a_frame_alone_gives_what_it_gives_in_the_batch(emul):
    case, painted = expected("odd")
    for f in range(2):
        one = dict(frames=case["frames"][f:f + 1], kp=case["kp"][f:f + 1], valid=case["valid"][f:f + 1], kw=case["kw"])
        got, y, uv = run(emul, one, "grid", "both")
        wy, wuv = surface_of("odd", "bt601", False, False)
        assert np.array_equal(got[0], painted[f]) and np.array_equal(y[0], wy[f]) and np.array_equal(uv[0], wuv[f])
    assert not np.array_equal(painted[0], painted[1])


def test_no_valid_no_scores_and_fewer_persons(emul):
    """P = 1 and P = 3 of the same figures, valid = NULL, C = 2 views of C = 3 keypoints: the restatement each time."""
    from tests.test_draw_cpu import draw_poses_np
    case, _ = expected("odd")
    for P in (1, 3):
        sub = dict(frames=case["frames"], kp=np.ascontiguousarray(case["kp"][:, :P, :, :2]), valid=None, kw={k: v for k, v in case["kw"].items() if k != "min_score"})
        want = draw_poses_np(sub["frames"], sub["kp"], None, **sub["kw"])
        got, y, uv = run(emul, sub, "odd", "both")
        wy, wuv = bgr_to_nv12_np(want)
        assert np.array_equal(got, want) and np.array_equal(y, wy) and np.array_equal(uv, wuv)


@pytest.mark.parametrize("Hf,Wf", [(1, 1), (2, 2), (3, 5), (7, 8), (16, 8), (37, 23), (33, 130)])
def test_no_primitives_is_bgr_to_nv12(emul, Hf, Wf):
    combos = itertools.cycle(COMBOS)
    for F in (1, 3):
        fr = noise_frames(F, Hf, Wf, 100 * Hf + Wf)
        case = dict(frames=fr, kp=None, valid=None, kw=dict(segments=np.zeros((0, 2), np.int32), colors=np.zeros((0, 3), np.uint8)))
        for place in ("grid", "odd", "pitch"):
            combo = next(combos)
            got, y, uv = run(emul, case, place, "surface", *combo)
            wy, wuv = bgr_to_nv12_np(fr, *combo)
            assert got is None and np.array_equal(y, wy) and np.array_equal(uv, wuv), (F, place, combo)
        got, y, uv = run(emul, case, "grid", "both")
        assert np.array_equal(got, fr), "nothing to paint: the frame is copied"


def test_pose_panel_source_equals_the_restatement(emul):
    from kasportsformer_amd.draw import panel_view
    g = np.random.default_rng(3)
    for n in (1, 5, 40):                                         # 40 * 17 = 680 joints: three blocks
        world = g.normal(0.0, 0.5, size=(n, 17, 3)).astype(np.float32)
        for rect, elev, azim in (((1280, 0, 1920, 640), 5.0, 5.0), ((3, 5, 90, 400), 15.0, 70.0)):
            view = panel_view(rect, elev, azim)
            buf = np.full(n * 34 + 16, np.float32(-7.0))
            keep = world.copy()
            assert emul.emul_pose_panel(world.ctypes.data, n, view.ctypes.data, buf[8:].ctypes.data) == 1
            assert np.array_equal(world, keep) and (buf[:8] == -7.0).all() and (buf[-8:] == -7.0).all()
            assert np.array_equal(buf[8:-8].reshape(n, 17, 2), pose_panel_np(world, view)), (n, rect)
