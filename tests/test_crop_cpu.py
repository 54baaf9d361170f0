"""Host side of the person crop (kasportsformer_amd.crop_persons, kasf_crop_persons): the numpy restatement of include/kasf.h's rules 1-5 that the GPU tests
hold the kernel to (tests/test_gpu_crop.py imports it from here), tied to what the reference's own box_to_center_scale and get_affine_transform and torch's
own ToTensor / Normalize arithmetic wrote into the fixture (tests/golden/make_crop_golden.py), and checked against exact fp64 bilinear sampling; the refusals of
the entry point and of the Python surface.  cv2.warpAffine itself could not be recorded (no OpenCV build at hand): rules 2-3 are tested as a sampling scheme
with a stated error bound, not as "the bits of cv2"."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_heatmap_cpu import box_to_center_scale_np, same_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64, I64 = np.float32, np.float64, np.int64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SAT = 2.0 ** 61


def fixture():
    return np.load(os.path.join(GOLDEN, "crop_persons.npz"), allow_pickle=False)


def fixture_frames(fx):
    """The two fixture frames as [2,Hf,Wf,3] uint8 VIEWS of the pitched buffer [2,Hf,pitch] (padding bytes are 255: a read into the padding shows)."""
    buf = fx["frames"]
    Hf, Wf = int(fx["frame_hw"][0]), int(fx["frame_hw"][1])
    return np.lib.stride_tricks.as_strided(buf, shape=(buf.shape[0], Hf, Wf, 3), strides=(buf.strides[0], buf.strides[1], 3, 1), writeable=False)


def crop_geometry_np(center, scale, out_w, out_h):
    """Rule 1 on float32 center, scale [P,2] -> kx, ky, bx, by, float64 [P]: crop pixel (x, y) sits at frame position (bx + kx x, by + ky y)."""
    center, scale = np.asarray(center, dtype=F32), np.asarray(scale, dtype=F32)
    cx, cy = center[:, 0], center[:, 1]
    with np.errstate(all="ignore"):
        sw = scale[:, 0] * F32(200)
        s1y = (cy.astype(F64) + (sw * F32(-0.5)).astype(F64)).astype(F32)
        dy = cy - s1y
        s2x = cx + (-dy)
        assert sw.dtype == dy.dtype == s2x.dtype == F32
        half_w, half_h = F64(out_w) * 0.5, F64(out_h) * 0.5
        kx = (cx.astype(F64) - s2x.astype(F64)) / half_w
        ky = (cy.astype(F64) - s1y.astype(F64)) / half_w
        bx = cx.astype(F64) - half_w * kx
        by = cy.astype(F64) - half_h * ky
    return kx, ky, bx, by


def _fix(v):
    """rint (half to even) to int64, saturated at +-2^61."""
    with np.errstate(all="ignore"):
        return np.clip(np.rint(v), -SAT, SAT).astype(I64)


def crop_positions_np(kx, ky, bx, by, out_w, out_h):
    """Rule 2 for one person -> X [out_w], Y [out_h] int64 on the 1/32-pixel grid (tap = >> 5, fraction = & 31)."""
    xs, ys = np.arange(out_w, dtype=F64), np.arange(out_h, dtype=F64)
    with np.errstate(all="ignore"):
        ad = _fix((kx * xs) * 1024.0)
        X0 = _fix(bx * 1024.0) + 16
        Y0 = _fix((ky * ys + by) * 1024.0) + 16
    return (X0 + ad) >> 5, Y0 >> 5


def normalise_table_np(mean=MEAN, std=STD):
    """Rule 4 for every value a channel can take: [3,256] float32, row c = the FRAME's channel c."""
    mean, std = np.asarray(mean, dtype=F32), np.asarray(std, dtype=F32)
    t = (np.arange(256, dtype=F32) / F32(255))[None, :]
    t = (t - mean[:, None]) / std[:, None]
    assert t.dtype == F32
    return t


def sample_np(frame, X, Y):
    """Rule 3: frame [Hf,Wf,3] uint8, positions of rule 2 -> v [out_h,out_w,3] int64 in 0..255."""
    Hf, Wf = frame.shape[:2]
    tx, fx, ty, fy = X >> 5, X & 31, Y >> 5, Y & 31

    def tap(dy, dx):
        yy, xx = ty + dy, tx + dx
        inside = ((yy >= 0) & (yy < Hf))[:, None] & ((xx >= 0) & (xx < Wf))[None, :]
        return frame[np.clip(yy, 0, Hf - 1)[:, None], np.clip(xx, 0, Wf - 1)[None, :], :].astype(I64) * inside[..., None]

    wx0, wx1, wy0, wy1 = (32 - fx)[None, :, None], fx[None, :, None], (32 - fy)[:, None, None], fy[:, None, None]
    S = wx0 * wy0 * tap(0, 0) + wx1 * wy0 * tap(0, 1) + wx0 * wy1 * tap(1, 0) + wx1 * wy1 * tap(1, 1)
    v = (S + 512) >> 10
    assert v.min() >= 0 and v.max() <= 255
    return v


def crop_persons_np(frame, boxes=None, *, center=None, scale=None, size=(288, 384), aspect=None, mean=MEAN, std=STD, swap_rb=True, frame_index=None,
                    parts=False):
    """kasf_crop_persons restated: frame [Hf,Wf,3] (or [F,Hf,Wf,3] with frame_index) uint8 -> (inputs [P,3,out_h,out_w] float32, center [P,2], scale [P,2]);
    with parts=True also the integer images v [P,out_h,out_w,3] before rule 4."""
    frame = np.asarray(frame)
    frames = frame if frame.ndim == 4 else frame[None]
    Hf, Wf = frames.shape[1:3]
    if boxes is not None:
        center, scale = box_to_center_scale_np(boxes, Hf / Wf if aspect is None else aspect)
    center, scale = np.asarray(center, dtype=F32), np.asarray(scale, dtype=F32)
    P, (out_w, out_h) = center.shape[0], size
    fi = np.zeros(P, I64) if frame_index is None else np.asarray(frame_index)
    kx, ky, bx, by = crop_geometry_np(center, scale, out_w, out_h)
    table = normalise_table_np(mean, std)
    out, vs = np.empty((P, 3, out_h, out_w), F32), np.zeros((P, out_h, out_w, 3), I64)
    for p in range(P):
        if np.isfinite([kx[p], ky[p], bx[p], by[p]]).all() and 0 <= fi[p] < frames.shape[0]:
            X, Y = crop_positions_np(kx[p], ky[p], bx[p], by[p], out_w, out_h)
            vs[p] = sample_np(frames[fi[p]], X, Y)
        for c in range(3):
            out[p, 2 - c if swap_rb else c] = table[c][vs[p, :, :, c]]
    return (out, center, scale, vs) if parts else (out, center, scale)


def exact_bilinear_np(frame, kx, ky, bx, by, out_w, out_h):
    """fp64 bilinear sampling of frame [Hf,Wf,3] at the UNQUANTISED positions (bx + kx x, by + ky y) -> (values [out_h,out_w,3] float64, interior [out_h,out_w]:
    all four taps inside the frame); values outside `interior` are meaningless."""
    Hf, Wf = frame.shape[:2]
    px, py = bx + kx * np.arange(out_w, dtype=F64), by + ky * np.arange(out_h, dtype=F64)
    x0, y0 = np.floor(px), np.floor(py)
    ax, ay = (px - x0)[None, :, None], (py - y0)[:, None, None]
    interior = ((y0 >= 0) & (y0 + 1 <= Hf - 1))[:, None] & ((x0 >= 0) & (x0 + 1 <= Wf - 1))[None, :]
    xi, yi = np.clip(x0, 0, Wf - 2).astype(I64), np.clip(y0, 0, Hf - 2).astype(I64)
    f = frame.astype(F64)
    val = ((1 - ax) * (1 - ay) * f[yi[:, None], xi[None, :]] + ax * (1 - ay) * f[yi[:, None], xi[None, :] + 1]
           + (1 - ax) * ay * f[yi[:, None] + 1, xi[None, :]] + ax * ay * f[yi[:, None] + 1, xi[None, :] + 1])
    return val, interior


def adjacent_difference(frame):
    f = frame.astype(I64)
    return int(max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max()))


def test_fixture_loads_without_pickles_and_is_small():
    path = os.path.join(GOLDEN, "crop_persons.npz")
    assert os.path.getsize(path) < 200 * 1024
    fx = fixture()
    Hf, Wf = (int(v) for v in fx["frame_hw"])
    assert (Hf, Wf) == (97, 131) and fx["frames"].dtype == np.uint8 and fx["frames"].shape[:2] == (2, Hf) and fx["frames"].shape[2] > 3 * Wf
    assert (fx["frames"][:, :, 3 * Wf:] == 255).all(), "the padding of the pitch is marked"
    fr = fixture_frames(fx)
    assert adjacent_difference(fr[0]) <= 16 < adjacent_difference(fr[1]), "a smooth frame and a noisy one"
    P = fx["boxes"].shape[0]
    assert P >= 12 and fx["boxes"].dtype == F32 and fx["ref_center"].shape == fx["ref_scale"].shape == (P, 2) and fx["ref_trans"].shape == (P, 2, 3)
    assert tuple(fx["size"]) == (24, 32) and fx["aspect"].dtype == F64 and float(fx["aspect"]) == Hf / Wf
    b, names = fx["boxes"], [str(s) for s in fx["names"]]
    assert len(names) == P and len(set(names)) == P
    for want in ("inside", "left", "right", "top", "bottom", "outside", "larger", "zero_width", "center_x_minus_1", "nan", "ties"):
        assert want in names, want
    assert np.isnan(b[names.index("nan")]).any() and b[names.index("zero_width")][0] == b[names.index("zero_width")][2]
    assert fx["ref_center"][names.index("center_x_minus_1"), 0] == -1
    assert fx["table_ref"].shape == (3, 256) and fx["table_ref"].dtype == F32


def test_box_path_gives_the_reference_center_and_scale_bit_for_bit():
    fx = fixture()
    c, s = box_to_center_scale_np(fx["boxes"], fx["aspect"])
    assert same_bits(c, fx["ref_center"]) and same_bits(s, fx["ref_scale"])
    out, c2, s2 = crop_persons_np(fixture_frames(fx)[0], fx["boxes"], size=tuple(fx["size"]))
    assert same_bits(c2, fx["ref_center"]) and same_bits(s2, fx["ref_scale"]), "aspect defaults to Hf / Wf in Python floats"
    i = [str(n) for n in fx["names"]].index("center_x_minus_1")
    grown = fx["boxes"][i, 3] - fx["boxes"][i, 1]
    assert s[i, 1] == F32(F64(grown) / 200), "center x == -1: no 1.25"


def test_inverse_map_is_the_fp64_inverse_of_the_reference_forward_matrix():
    """get_affine_transform(center, scale, 0, size) is the FORWARD map (frame -> crop) that cv2.warpAffine inverts; its fp64 inverse against rule 1's closed form,
    1e-12 relative to the size of each coefficient's row (the off-diagonal terms are 0 in the closed form)."""
    fx = fixture()
    out_w, out_h = (int(v) for v in fx["size"])
    kx, ky, bx, by = crop_geometry_np(fx["ref_center"], fx["ref_scale"], out_w, out_h)
    checked = 0
    for p, m in enumerate(fx["ref_trans"]):
        if not np.isfinite(m).all():
            continue                                            # the NaN box and the zero-size box: the reference's forward matrix does not exist
        full = np.vstack((m, [0.0, 0.0, 1.0]))
        inv = np.linalg.inv(full)[:2]
        mine = np.array([[kx[p], 0.0, bx[p]], [0.0, ky[p], by[p]]])
        tol = 1e-12 * np.abs(mine).max(axis=1, keepdims=True)
        assert (np.abs(inv - mine) <= tol).all(), (p, inv, mine)
        checked += 1
    assert checked >= 10


def test_normalise_table_is_torchs_bit_for_bit():
    fx = fixture()
    t = normalise_table_np()
    assert same_bits(t, fx["table_ref"]), "all 768 entries against the recorded ToTensor / Normalize values"
    v = torch.arange(256, dtype=torch.uint8)
    for c in range(3):
        assert same_bits(t[c], v.float().div(255).sub(MEAN[c]).div(STD[c]).numpy())


def test_ties_person_sits_on_half_grid_ties_and_rounds_to_even():
    fx = fixture()
    out_w, out_h = (int(v) for v in fx["size"])
    i = [str(n) for n in fx["names"]].index("ties")
    kx, ky, bx, by = (v[i] for v in crop_geometry_np(fx["ref_center"], fx["ref_scale"], out_w, out_h))
    tx = (kx * np.arange(out_w, dtype=F64)) * 1024.0
    ty = (ky * np.arange(out_h, dtype=F64) + by) * 1024.0
    assert (np.abs(tx - np.floor(tx)) == 0.5).sum() >= out_w // 2 and (np.abs(ty - np.floor(ty)) == 0.5).sum() >= out_h // 2
    assert (_fix(tx) % 2 == 0)[np.abs(tx - np.floor(tx)) == 0.5].all(), "half to even"
    assert _fix(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e300, -1e300])).tolist() == [0, 2, 2, 0, -2, 2 ** 61, -2 ** 61]


def accuracy_persons(fx):
    """The fixture's boxes and 188 seeded ones mostly inside the frame: 200 persons."""
    g = np.random.default_rng(77)
    Hf, Wf = (int(v) for v in fx["frame_hw"])
    n = 200 - fx["boxes"].shape[0]
    cx, cy = g.uniform(0.3 * Wf, 0.7 * Wf, n), g.uniform(0.3 * Hf, 0.7 * Hf, n)
    bw, bh = g.uniform(2, 0.45 * Wf, n), g.uniform(2, 0.45 * Hf, n)
    more = np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), axis=-1).astype(F32)
    return np.concatenate((fx["boxes"], more))


def test_sampling_is_bilinear_at_the_stated_positions_within_the_grid_error():
    """On the smooth frame, every output pixel whose taps all lie inside the frame in both versions: |v - exact| <= 0.5 + G / 16 with G the frame's largest
    adjacent-pixel difference -- 1/32 px of position error per axis plus the final rounding.  A half-pixel or swapped-axis mistake gives about G / 2.  At least
    30 % of all sampled pixels must be such interior pixels."""
    fx = fixture()
    frame = fixture_frames(fx)[0]
    Hf, Wf = frame.shape[:2]
    out_w, out_h = (int(v) for v in fx["size"])
    G = adjacent_difference(frame)
    assert G <= 16
    boxes = accuracy_persons(fx)
    _, center, scale, vs = crop_persons_np(frame, boxes, size=(out_w, out_h), parts=True)
    kx, ky, bx, by = crop_geometry_np(center, scale, out_w, out_h)
    worst, used, total = 0.0, 0, 0
    for p in range(boxes.shape[0]):
        total += out_w * out_h
        if not np.isfinite([kx[p], ky[p], bx[p], by[p]]).all():
            continue
        exact, interior = exact_bilinear_np(frame, kx[p], ky[p], bx[p], by[p], out_w, out_h)
        X, Y = crop_positions_np(kx[p], ky[p], bx[p], by[p], out_w, out_h)
        tx, ty = X >> 5, Y >> 5
        interior &= ((ty >= 0) & (ty + 1 <= Hf - 1))[:, None] & ((tx >= 0) & (tx + 1 <= Wf - 1))[None, :]
        if interior.any():
            worst = max(worst, float(np.abs(vs[p] - exact)[interior].max()))
        used += int(interior.sum())
    bound = 0.5 + G / 16
    print(f"quantised vs exact bilinear: worst {worst:.3f}, bound {bound:.3f} (G = {G}); interior {used} of {total} pixels")
    assert used >= 0.30 * total, (used, total)
    assert worst <= bound, (worst, bound)


def test_border_swap_and_degenerate_persons():
    fx = fixture()
    frames, names = fixture_frames(fx), [str(n) for n in fx["names"]]
    size = tuple(int(v) for v in fx["size"])
    out, c, s, vs = crop_persons_np(frames[1], fx["boxes"], size=size, parts=True)
    table = normalise_table_np()
    for name in ("outside", "nan"):
        i = names.index(name)
        assert not vs[i].any(), name
        for k in range(3):
            assert (out[i, k] == table[2 - k][0]).all(), "border = the normalised value of 0; plane k is frame channel 2 - k"
    i = names.index("zero_size")
    assert (vs[i] == vs[i][0, 0]).all() and vs[i].any(), "kx = ky = 0: one frame position everywhere"
    for name in ("left", "right", "top", "bottom", "larger"):
        v = vs[names.index(name)]
        assert v.any() and not v.all(axis=-1).all(), f"{name}: part frame, part border"
    plain = crop_persons_np(frames[1], fx["boxes"], size=size, swap_rb=False)[0]
    assert same_bits(plain[:, ::-1], out)
    other = crop_persons_np(frames[1], fx["boxes"], size=size, mean=(0.1, 0.2, 0.3), std=(0.5, 2.0, -1.5))[0]
    i = names.index("inside")
    assert same_bits(other[i, 2], ((vs[i, :, :, 0].astype(F32) / F32(255)) - F32(0.1)) / F32(0.5))
    cs = crop_persons_np(frames[1], center=c, scale=s, size=size)[0]
    keep = ~np.isnan(c).any(axis=1)
    assert same_bits(cs[keep], out[keep])
    both = crop_persons_np(frames, np.concatenate((fx["boxes"], fx["boxes"])), size=size, frame_index=np.repeat([1, 0], len(names)))[0]
    assert same_bits(both[:len(names)], out) and not same_bits(both[len(names):], out)


def entry_args(**over):
    """Host buffers and the argument list of kasf_crop_persons for one person of a 5 x 7 frame -> (call, buffers)."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    frame, geom = np.full(5 * 7 * 3, 3, np.uint8), np.full(4, 5, F32)
    out, cs, idx = np.full(3 * 4 * 6, 7, F32), np.full(4, 9, F32), np.zeros(1, np.int32)
    ms = np.array(MEAN + STD, F32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(frames=vp(frame), n_frames=1, Hf=5, Wf=7, row_stride=21, frame_stride=105, frame_index=None, geom=vp(geom), kind=0, aspect=1.0, n=1, out=vp(out),
             dtype=0, out_w=6, out_h=4, mean_std=ms, swap=1, cs=vp(cs)):
        m = None if mean_std is None else np.ascontiguousarray(mean_std, dtype=F32).ctypes.data_as(C.POINTER(C.c_float))
        return lib.kasf_crop_persons(frames, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, kind, aspect, n, out, dtype, out_w, out_h, m, swap, cs, None)

    return call, (frame, geom, out, cs, idx)


REFUSED = [dict(n=-1), dict(out_w=0), dict(out_h=0), dict(out_w=-3), dict(out_h=32768), dict(Hf=0), dict(Wf=0), dict(Hf=32768), dict(Wf=32768, row_stride=3 * 32768),
           dict(Hf=-1), dict(row_stride=20), dict(row_stride=0), dict(row_stride=-21), dict(n_frames=0), dict(n_frames=2, frame_stride=-105, frame_index="idx"),
           dict(dtype=3), dict(dtype=-1), dict(kind=2), dict(kind=-1), dict(kind=1, aspect=0.0), dict(kind=1, aspect=-0.5), dict(kind=1, aspect=float("nan")),
           dict(mean_std=MEAN + (0.229, 0.0, 0.225)), dict(mean_std=MEAN + (float("inf"), 0.224, 0.225)), dict(mean_std=MEAN + (0.229, 0.224, float("nan"))),
           dict(mean_std=None), dict(frames=None), dict(geom=None), dict(out=None), dict(n_frames=2, frame_index=None)]


def test_entry_point_refuses_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    assert "kasf_crop_persons" in _lib.SIGNATURES and hasattr(lib, "kasf_crop_persons")
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "kasf.h")).read()
    assert "int kasf_crop_persons(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride," in hdr
    assert "equality with a particular cv2 build is unverified" in hdr
    assert _lib.ABI_VERSION == lib.kasf_version() == 12
    call, (frame, geom, out, cs, idx) = entry_args()
    assert call(n=0) == 0 and call(frames=None, n=0, geom=None, out=None, cs=None) == 0          # nothing to do
    for kw in REFUSED:
        kw = {k: (idx.ctypes.data_as(C.c_void_p) if v == "idx" else v) for k, v in kw.items()} if "frame_index" in kw else kw
        assert call(**kw) == 2, kw
        assert lib.kasf_last_error(), kw
    assert (frame == 3).all() and (geom == 5).all() and (out == 7).all() and (cs == 9).all(), "a refused call touches no buffer"


def test_python_surface_refuses_before_any_launch():
    import kasportsformer_amd as K
    assert "crop_persons" in K.__all__ and "crop_persons" in K.__doc__ and "CropResult" in K.__all__
    frame = np.zeros((9, 11, 3), np.uint8)
    b, c, s = np.array([[0, 0, 4, 4]] * 2, F32), np.zeros((2, 2), F32), np.ones((2, 2), F32)
    with pytest.raises(RuntimeError):
        K.crop_persons(frame, b, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.crop_persons(frame, b)
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.crop_persons(torch.zeros((2, 9, 11, 3), dtype=torch.uint8), center=c, scale=s, frame_index=[0, 1], dtype=torch.bfloat16, size=(5, 3))
    f = K.crop_persons
    for exc, call in ((TypeError, lambda: f(frame.astype(F32), b)),
                      (TypeError, lambda: f(frame.tolist(), b)),
                      (TypeError, lambda: f(torch.zeros((9, 11, 3)), b)),
                      (TypeError, lambda: f(frame, b.astype(F64))),
                      (TypeError, lambda: f(frame, center=c.astype(np.float16), scale=s)),
                      (TypeError, lambda: f(frame, b, dtype=torch.float64)),
                      (TypeError, lambda: f(frame, b, size=7)),
                      (TypeError, lambda: f(frame[None], b, frame_index=np.zeros(2, F32))),
                      (ValueError, lambda: f(frame[:, :, :2], b)),
                      (ValueError, lambda: f(frame[0], b)),
                      (ValueError, lambda: f(frame[:0], b)),
                      (ValueError, lambda: f(frame)),
                      (ValueError, lambda: f(frame, center=c)),
                      (ValueError, lambda: f(frame, b, center=c, scale=s)),
                      (ValueError, lambda: f(frame, center=c, scale=s[:1])),
                      (ValueError, lambda: f(frame, center=c, scale=s, aspect=1.0)),
                      (ValueError, lambda: f(frame, b[:, :3])),
                      (ValueError, lambda: f(frame, b[0])),
                      (ValueError, lambda: f(frame, b, aspect=0.0)),
                      (ValueError, lambda: f(frame, b, aspect=float("inf"))),
                      (ValueError, lambda: f(frame, b, size=(0, 4))),
                      (ValueError, lambda: f(frame, b, size=(4, 40000))),
                      (ValueError, lambda: f(frame, b, std=(0.2, 0.0, 0.2))),
                      (ValueError, lambda: f(frame, b, std=(0.2, 0.2))),
                      (ValueError, lambda: f(frame, b, mean=(0.1, float("nan"), 0.2))),
                      (ValueError, lambda: f(frame, b, frame_index=[0, 0])),
                      (ValueError, lambda: f(frame[None], b)),
                      (ValueError, lambda: f(frame[None], b, frame_index=[0])),
                      (ValueError, lambda: f(frame[None], b, frame_index=[0, 1])),
                      (ValueError, lambda: f(frame[None], b, frame_index=[-1, 0]))):
        with pytest.raises(exc):
            call()
    assert not frame.any() and not c.any()
