"""The decoder-surface conversion (kasf_yuv420_to_bgr, K.yuv_to_bgr / nv12_to_bgr / i420_to_bgr) without a GPU: `yuv_to_bgr_np`, the numpy restatement of
include/kasf.h's rules that the host-emulation and GPU tests hold the kernel to bit for bit, and what ties the restatement itself down:

  accuracy   for each of the four coefficient tables, over ALL 2^24 (Y, U, V), every channel within a bound of the exact fp64 conversion built from Kr, Kb
             and the range scales.  The bound is computed from the table, not measured: 0.5 for the final rounding + sum |c_int / 2^20 - c_exact| * max|operand|.
  tables     the header's literals against rint(c * 2^20) of the formulas of rule 4 (BT.601 limited against OpenCV's five published constants).
  siting     odd sizes against a per-pixel loop; NV12 and I420 of the same samples give the same bytes.
  refusals   every refusal of the Python argument checks that needs no device, and every error-2 refusal of the C entry point (which touches no pointer).

NOT verified here or anywhere: equality with a particular cv2 / FFmpeg build (there is no OpenCV at hand)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rule 4: { CY, CVR, CVG, CUG, CUB } per (matrix, full_range)
TABLES = {
    ("bt601", False): (1220542, 1673527, -852492, -409993, 2116026),          # OpenCV's published constants: 1.164, 1.596, 0.813, 0.391, 2.018
    ("bt601", True): (1048576, 1470104, -748826, -360853, 1858077),
    ("bt709", False): (1220945, 1879825, -558796, -223607, 2215014),
    ("bt709", True): (1048576, 1651297, -490864, -196424, 1945738),
}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SIZES = ((1, 1), (2, 2), (3, 5), (5, 3), (7, 8), (16, 8), (37, 23))             # (Hf, Wf): odd sizes, fewer than 8 columns, whole blocks with and without a remainder


def exact_coefficients(matrix, full_range):
    """The five exact doubles of rule 4 from Kr, Kb, the luma scale and the chroma scale."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    ls, cs = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return (ls, 2.0 * (1.0 - kr) * cs, -2.0 * (1.0 - kr) * kr / kg * cs, -2.0 * (1.0 - kb) * kb / kg * cs, 2.0 * (1.0 - kb) * cs)


def samples_to_bgr(Y, U, V, matrix="bt601", full_range=False):
    """Rule 3 on integer arrays that broadcast against each other -> (B, G, R) int32 in 0..255."""
    cy, cvr, cvg, cug, cub = (np.int32(c) for c in TABLES[(matrix, bool(full_range))])
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    y1 = (Y if full_range else np.maximum(0, Y - 16)) * cy
    u, v = U - 128, V - 128
    half = np.int32(1 << 19)
    r = np.clip((y1 + cvr * v + half) >> 20, 0, 255)             # int32 throughout: |sum| < 2^31 (kasf.h, rule 3); >> on int32 is arithmetic
    g = np.clip((y1 + cvg * v + cug * u + half) >> 20, 0, 255)
    b = np.clip((y1 + cub * u + half) >> 20, 0, 255)
    return b, g, r


def yuv_to_bgr_np(y, c0, c1=None, layout="nv12", matrix="bt601", full_range=False, rgb=False):
    """The numpy restatement of kasf_yuv420_to_bgr: y [Hf,Wf] uint8, c0 [ch,cw,2] (nv12) or c0, c1 [ch,cw] (i420), or all with a leading F -> uint8
    [Hf,Wf,3] / [F,Hf,Wf,3], channels B, G, R (R, G, B with rgb)."""
    y, c0 = np.asarray(y), np.asarray(c0)
    Hf, Wf = y.shape[-2:]
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    if layout == "nv12":
        assert c1 is None and c0.shape == y.shape[:-2] + (ch, cw, 2), (y.shape, c0.shape)
        U, V = c0[..., 0], c0[..., 1]
    else:
        c1 = np.asarray(c1)
        assert layout == "i420" and c0.shape == c1.shape == y.shape[:-2] + (ch, cw), (y.shape, c0.shape)
        U, V = c0, c1
    yy, xx = np.arange(Hf) >> 1, np.arange(Wf) >> 1                                      # rule 2: pixel (y, x) takes chroma sample (y >> 1, x >> 1)
    U, V = U[..., yy[:, None], xx[None, :]], V[..., yy[:, None], xx[None, :]]
    b, g, r = samples_to_bgr(y, U, V, matrix, full_range)
    return np.stack((r, g, b) if rgb else (b, g, r), axis=-1).astype(np.uint8)


def nv12_planes_np(surface, height=None, width=None, chroma_row=None):
    """(y, uv) views of an NV12 surface [rows, pitch] (or [F, rows, pitch]), by K.nv12_to_bgr's defaults."""
    surface = np.asarray(surface)
    rows, pitch = surface.shape[-2:]
    Hf = rows * 2 // 3 if height is None else height
    Wf = pitch if width is None else width
    cr = Hf if chroma_row is None else chroma_row
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    uv = surface[..., cr:cr + ch, :2 * cw]
    return surface[..., :Hf, :Wf], uv.reshape(uv.shape[:-1] + (cw, 2))


def nv12_to_bgr_np(surface, height=None, width=None, chroma_row=None, **kw):
    return yuv_to_bgr_np(*nv12_planes_np(surface, height, width, chroma_row), layout="nv12", **kw)


def i420_planes_np(surface, height=None, width=None, chroma_row=None):
    """(y, u, v) of a packed I420 surface [rows, pitch]: U as ch rows of pitch / 2 bytes from chroma_row, V right behind it."""
    surface = np.ascontiguousarray(surface)
    rows, pitch = surface.shape[-2:]
    Hf = rows * 2 // 3 if height is None else height
    Wf = pitch if width is None else width
    cr = Hf if chroma_row is None else chroma_row
    ch, cw, half = Hf // 2, Wf // 2, pitch // 2
    flat = surface.reshape(surface.shape[:-2] + (-1,))
    u = flat[..., cr * pitch:cr * pitch + ch * half].reshape(flat.shape[:-1] + (ch, half))[..., :cw]
    v = flat[..., cr * pitch + ch * half:cr * pitch + 2 * ch * half].reshape(flat.shape[:-1] + (ch, half))[..., :cw]
    return surface[..., :Hf, :Wf], u, v


def noise_planes(Hf, Wf, seed, frames=None):
    """Seeded 0..255 noise planes (y, u, v) with the extremes forced in: [Hf,Wf], [ch,cw], [ch,cw] (a leading `frames` if given)."""
    g = np.random.default_rng(seed)
    lead = () if frames is None else (frames,)
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    y, u, v = (g.integers(0, 256, size=lead + s, dtype=np.uint8) for s in ((Hf, Wf), (ch, cw), (ch, cw)))
    y[..., 0, 0], u[..., 0, 0], v[..., 0, 0] = 255, 0, 255
    y[..., -1, -1], u[..., -1, -1], v[..., -1, -1] = 0, 255, 0
    return y, u, v


def interleave(u, v):
    return np.ascontiguousarray(np.stack((u, v), axis=-1))


# ---- accuracy: all 2^24 samples ----
def worst_distance(table, exact):
    """max over all 2^24 (Y, U, V) of |restatement with `table` - exact fp64 conversion with `exact`| per channel (B, G, R); table, exact = (matrix, full_range)."""
    ls, cvr, cvg, cug, cub = exact_coefficients(*exact)
    U, V = np.arange(256)[:, None], np.arange(256)[None, :]
    u, v = (U - 128).astype(np.float64), (V - 128).astype(np.float64)
    worst = np.zeros(3)
    for Y in range(256):
        b, g, r = samples_to_bgr(Y, U, V, *table)
        y1 = ls * (Y if exact[1] else max(0, Y - 16))
        want = (np.clip(y1 + cub * u, 0, 255), np.clip(y1 + cvg * v + cug * u, 0, 255), np.clip(y1 + cvr * v, 0, 255))
        for c, (got, w) in enumerate(zip((b, g, r), want)):
            worst[c] = max(worst[c], float(np.abs(got - w).max()))                        # (got broadcasts to the 256 x 256 grid)
    return worst


def bounds(matrix, full_range):
    """(bound of the issue = 0.5 + the sum over all five coefficients, per-channel bounds B, G, R = 0.5 + the sum over that channel's coefficients)."""
    d = [abs(ci / 2.0 ** 20 - ce) for ci, ce in zip(TABLES[(matrix, full_range)], exact_coefficients(matrix, full_range))]
    luma = 255.0 if full_range else 239.0                                                # max(0, Y - 16) <= 239
    dy, dvr, dvg, dug, dub = d[0] * luma, d[1] * 128.0, d[2] * 128.0, d[3] * 128.0, d[4] * 128.0
    return 0.5 + dy + dvr + dvg + dug + dub, (0.5 + dy + dub, 0.5 + dy + dvg + dug, 0.5 + dy + dvr)


EPS = 1e-9        # the fp64 evaluation of the exact conversion itself (a few ulp of 300)


@pytest.mark.parametrize("matrix,full_range", sorted(TABLES))
def test_every_sample_is_within_the_computed_bound_of_the_exact_conversion(matrix, full_range):
    """Bounds (all five coefficients / per channel B, G, R) and the measured worst distances (B, G, R):
      bt601 limited  0.7952 / 0.6900 0.6935 0.5952   measured 0.6750 0.6905 0.5892
      bt601 full     0.5001 / 0.5000 0.5000 0.5001   measured 0.5000 0.5000 0.4980
      bt709 limited  0.5002 / 0.5001 0.5001 0.5001   measured 0.5000 0.5001 0.5001
      bt709 full     0.5002 / 0.5000 0.5000 0.5001   measured 0.4980 0.5000 0.4964"""
    total, per_channel = bounds(matrix, full_range)
    worst = worst_distance((matrix, full_range), (matrix, full_range))
    print(f"{matrix} full_range={full_range}: bound {total:.4f}, per channel B, G, R {['%.4f' % b for b in per_channel]}, measured {['%.4f' % w for w in worst]}")
    assert total < (0.8 if (matrix, full_range) == ("bt601", False) else 0.5003)
    for w, b in zip(worst, per_channel):
        assert w <= b + EPS <= total + EPS, (worst, per_channel, total)


def test_a_wrong_matrix_or_range_violates_the_bound():
    """The accuracy test can see the difference: the BT.601 limited restatement against the exact BT.709 limited conversion is 12.43 (B) / 59.08 (G) /
    25.59 (R) grey levels away at worst, against the exact BT.601 full conversion 30.73 / 20.88 / 24.95; the bound is 0.80."""
    total, _ = bounds("bt601", False)
    matrix = worst_distance(("bt601", False), ("bt709", False))
    rng = worst_distance(("bt601", False), ("bt601", True))
    print("wrong matrix:", matrix, "wrong range:", rng)
    assert matrix.min() > total and rng.min() > total, "every channel violates the bound"


# ---- the tables ----
def header_tables():
    hdr = open(os.path.join(ROOT, "include", "kasf.h")).read()
    found = {}
    for m in re.finditer(r"#define\s+KASF_YUV_COEF_(BT601|BT709)_(LIMITED|FULL)\s*\{([^}]*)\}", hdr):
        found[(m[1].lower(), m[2] == "FULL")] = tuple(int(v) for v in m[3].split(","))
    return hdr, found


def test_header_literals_are_the_rounded_formulas():
    hdr, found = header_tables()
    assert found == TABLES, "include/kasf.h and the restatement hold the same four tables"
    for key in (("bt601", True), ("bt709", False), ("bt709", True)):
        assert found[key] == tuple(int(np.rint(c * 2.0 ** 20)) for c in exact_coefficients(*key)), key
    assert found[("bt601", False)] == tuple(int(np.rint(c * 2.0 ** 20)) for c in (1.164, 1.596, -0.813, -0.391, 2.018)), "OpenCV's published constants"
    for name, value in (("KASF_YUV_NV12", 0), ("KASF_YUV_I420", 1), ("KASF_YUV_BT601", 0), ("KASF_YUV_BT709", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", hdr), name
    from kasportsformer_amd import _lib, yuv
    assert (_lib.YUV_NV12, _lib.YUV_I420, _lib.YUV_BT601, _lib.YUV_BT709) == (0, 1, 0, 1)
    assert yuv.LAYOUTS == {"nv12": 0, "i420": 1} and yuv.MATRICES == {"bt601": 0, "bt709": 1}
    # rule 3's bound: every intermediate fits int32
    for (matrix, full), (cy, cvr, cvg, cug, cub) in TABLES.items():
        luma = 255 * cy
        assert luma + 128 * max(abs(cvr), abs(cub), abs(cvg) + abs(cug)) + (1 << 19) < 5.97e8 < 2 ** 31


# ---- siting and layouts ----
@pytest.mark.parametrize("Hf,Wf", SIZES)
def test_nearest_siting_on_odd_sizes_and_both_layouts(Hf, Wf):
    y, u, v = noise_planes(Hf, Wf, seed=Hf * 100 + Wf)
    assert u.shape == ((Hf + 1) // 2, (Wf + 1) // 2)
    for (matrix, full) in TABLES:
        want = np.zeros((Hf, Wf, 3), np.uint8)
        for yy in range(Hf):
            for xx in range(Wf):                                                         # the last column / row of an odd size shares the last chroma sample
                want[yy, xx] = [int(c) for c in samples_to_bgr(y[yy, xx], u[yy >> 1, xx >> 1], v[yy >> 1, xx >> 1], matrix, full)]
        planar = yuv_to_bgr_np(y, u, v, layout="i420", matrix=matrix, full_range=full)
        semi = yuv_to_bgr_np(y, interleave(u, v), matrix=matrix, full_range=full)
        assert planar.dtype == np.uint8 and np.array_equal(planar, want) and np.array_equal(semi, want)
        assert np.array_equal(yuv_to_bgr_np(y, u, v, layout="i420", matrix=matrix, full_range=full, rgb=True), want[..., ::-1])


def test_grey_levels():
    """Limited-range grey (U = V = 128) maps 16 -> 0, 235 -> 255 and 126 -> 128 in every channel; full range is the identity on grey."""
    for matrix in ("bt601", "bt709"):
        for Y, want in ((16, 0), (235, 255), (126, 128), (0, 0), (255, 255)):
            assert [int(c) for c in samples_to_bgr(Y, 128, 128, matrix, False)] == [want] * 3
        for Y in (0, 1, 77, 254, 255):
            assert [int(c) for c in samples_to_bgr(Y, 128, 128, matrix, True)] == [Y] * 3


def test_surfaces_and_batches():
    y, u, v = noise_planes(6, 10, seed=4, frames=3)
    all_ = yuv_to_bgr_np(y, interleave(u, v))
    assert all_.shape == (3, 6, 10, 3)
    for f in range(3):
        assert np.array_equal(all_[f], yuv_to_bgr_np(y[f], u[f], v[f], layout="i420"))
    surf = np.full((8 + 3, 16), 7, np.uint8)                                             # 6 luma rows aligned to 8, pitch 16
    surf[:6, :10], surf[8:11, :10] = y[0], interleave(u[0], v[0]).reshape(3, 10)
    assert np.array_equal(nv12_to_bgr_np(surf, 6, 10, chroma_row=8), all_[0])
    packed = np.concatenate((y[1].reshape(-1), u[1].reshape(-1), v[1].reshape(-1))).reshape(9, 10)          # yuv420p in one buffer
    assert np.array_equal(yuv_to_bgr_np(*i420_planes_np(packed), layout="i420"), all_[1])
    from kasportsformer_amd.yuv import surface_planes
    ys, uvs = surface_planes(surf, 6, 10, 8, "nv12", "t")
    assert ys.data_ptr() == surf.ctypes.data and np.array_equal(yuv_to_bgr_np(ys.numpy(), uvs.numpy()), all_[0]), "the planes are views of the surface"
    yp, up, vp = surface_planes(packed, None, None, None, "i420", "t")
    assert np.array_equal(yuv_to_bgr_np(yp.numpy(), up.numpy(), vp.numpy(), layout="i420"), all_[1])
    batch = np.stack([packed, packed])
    yb, ub, vb = surface_planes(batch, None, None, None, "i420", "t")
    assert tuple(yb.shape) == (2, 6, 10) and tuple(ub.shape) == (2, 3, 5) and np.array_equal(vb[1].numpy(), v[1])


# ---- refusals that need no device ----
def test_python_refusals_need_no_device():
    import kasportsformer_amd as K
    from kasportsformer_amd.yuv import check_yuv_args, surface_planes
    y, u, v = noise_planes(6, 10, seed=1)
    uv = interleave(u, v)

    def chk(*a, layout="nv12", matrix="bt601", out=None):
        args = (a + (None,))[:3]
        return check_yuv_args(*args, layout, matrix, out, "t")

    yt, c0, c1, lay, mat, o, batched = chk(y, uv)
    assert tuple(yt.shape) == (1, 6, 10) and tuple(c0.shape) == (1, 3, 5, 2) and c1 is None and (lay, mat, o, batched) == (0, 0, None, False)
    yt, c0, c1, lay, mat, o, batched = chk(y[None], u[None], v[None], layout="i420", matrix="bt709")
    assert tuple(c1.shape) == (1, 3, 5) and (lay, mat, batched) == (1, 1, True)
    with pytest.raises(TypeError):
        chk(y.astype(np.int32), uv)
    with pytest.raises(TypeError):
        chk(y, uv.astype(np.float32))
    with pytest.raises(TypeError):
        chk(y, u, v.astype(np.int16), layout="i420")
    with pytest.raises(TypeError):
        chk(y.tolist(), uv)
    with pytest.raises(TypeError):
        chk(torch.from_numpy(y).float(), uv)
    for bad in ("nv21", "NV12", None, 0):
        with pytest.raises(ValueError):
            chk(y, uv, layout=bad)
    for bad in ("bt2020", "601", None):
        with pytest.raises(ValueError):
            chk(y, uv, matrix=bad)
    with pytest.raises(ValueError):
        chk(y, uv, v)                                            # nv12 with a separate v
    with pytest.raises(ValueError):
        chk(y, u, layout="i420")                                 # i420 without v
    with pytest.raises(ValueError):
        chk(y, u)                                                # nv12 chroma without the pair dimension
    with pytest.raises(ValueError):
        chk(y, uv[:2])                                           # too few chroma rows
    with pytest.raises(ValueError):
        chk(y, u, v[:, :4], layout="i420")
    with pytest.raises(ValueError):
        chk(y[None], uv)                                         # a batch of luma, one chroma plane
    with pytest.raises(ValueError):
        chk(y[0], uv)                                            # y is not a plane
    with pytest.raises(ValueError):
        chk(np.zeros((0, 10), np.uint8), np.zeros((0, 5, 2), np.uint8))
    with pytest.raises(ValueError):
        chk(np.zeros((1, 32768), np.uint8), np.zeros((1, 16384, 2), np.uint8))
    with pytest.raises(TypeError):
        chk(y, uv, out=np.zeros((6, 10, 3), np.uint8))           # out is a torch tensor
    with pytest.raises(TypeError):
        chk(y, uv, out=torch.zeros((6, 10, 3)))                  # of uint8
    with pytest.raises(ValueError):
        chk(y, uv, out=torch.zeros((6, 10, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        chk(y, uv, out=torch.zeros((1, 6, 10, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        chk(y, uv, out=torch.zeros((6, 10, 3), dtype=torch.uint8))           # on the host
    with pytest.raises(RuntimeError):
        K.yuv_to_bgr(y, uv, device="cpu")
    with pytest.raises(RuntimeError):
        K.nv12_to_bgr(np.zeros((9, 10), np.uint8), device="cpu")
    with pytest.raises(RuntimeError):
        K.i420_to_bgr(np.zeros((9, 10), np.uint8), device="cpu")
    # surfaces
    surf = np.zeros((9, 10), np.uint8)
    assert [tuple(p.shape) for p in surface_planes(surf, None, None, None, "nv12", "t")] == [(6, 10), (3, 5, 2)]
    assert [tuple(p.shape) for p in surface_planes(surf, 5, 7, 6, "nv12", "t")] == [(5, 7), (3, 4, 2)]
    with pytest.raises(TypeError):
        surface_planes(surf.astype(np.int8), None, None, None, "nv12", "t")
    with pytest.raises(TypeError):
        surface_planes(surf, 6.0, None, None, "nv12", "t")
    with pytest.raises(TypeError):
        surface_planes(surf, 6, True, None, "nv12", "t")
    with pytest.raises(ValueError):
        surface_planes(surf[0], None, None, None, "nv12", "t")
    with pytest.raises(ValueError):
        surface_planes(surf, 8, None, None, "nv12", "t")        # 8 + 4 rows needed
    with pytest.raises(ValueError):
        surface_planes(surf, 6, 11, None, "nv12", "t")          # wider than the pitch
    with pytest.raises(ValueError):
        surface_planes(surf, 6, 10, 5, "nv12", "t")             # chroma inside the luma rows
    with pytest.raises(ValueError):
        surface_planes(surf, 6, 10, 7, "nv12", "t")             # 7 + 3 rows needed
    with pytest.raises(ValueError):
        surface_planes(surf, 0, 10, None, "nv12", "t")
    with pytest.raises(ValueError):
        surface_planes(np.zeros((8, 9), np.uint8), 5, 9, None, "i420", "t")          # odd sizes have no packed I420
    with pytest.raises(ValueError):
        surface_planes(surf, 6, 10, 8, "i420", "t")


# ---- the C entry point's refusals: error 2 before a device or a pointer is touched ----
# the accepted call they start from: NV12, two frames of 5 x 7 behind pitches of 8 (luma, chroma) and 21 (output)
ACCEPTED = dict(layout=0, n_frames=2, Hf=5, Wf=7, y_row_stride=8, c_row_stride=8, y_frame_stride=40, c_frame_stride=24, out_row_stride=21,
                out_frame_stride=105, matrix=0, c1=False)
REFUSED = [                                                      # (what differs from ACCEPTED, a word of the message it must give)
    (dict(n_frames=-1), "n_frames"),
    (dict(Hf=0), "Hf and Wf"), (dict(Hf=32768), "Hf and Wf"), (dict(Wf=0), "Hf and Wf"), (dict(Wf=32768), "Hf and Wf"), (dict(Hf=-3), "Hf and Wf"),
    (dict(y_row_stride=6), "luma row stride"),
    (dict(c_row_stride=7), "chroma row stride"),                                                  # NV12: 2 * cw = 8
    (dict(layout=1, c1=True, c_row_stride=3), "chroma row stride"),                               # I420: cw = 4
    (dict(out_row_stride=20), "output row stride"),
    (dict(y_frame_stride=-1), "frame strides"), (dict(c_frame_stride=-1), "frame strides"), (dict(out_frame_stride=-1), "frame strides"),
    (dict(n_frames=1, y_frame_stride=-8), "frame strides"),
    (dict(y_frame_stride=39), "cover its plane"), (dict(c_frame_stride=23), "cover its plane"), (dict(out_frame_stride=104), "cover its plane"),
    (dict(y_row_stride=2 ** 62, y_frame_stride=2 ** 62), "cover its plane"),                       # (no overflow in the check itself)
    (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
    (dict(matrix=2), "matrix"), (dict(matrix=-1), "matrix"),
    (dict(c1=True), "c1"),                                                                        # NV12 with a V plane
    (dict(layout=1, c_row_stride=4, c_frame_stride=12), "c1"),                                    # I420 without one
]
NULLS = ("y", "c0", "out")                                       # each null alone, with n_frames > 0 and everything else accepted: "null pointer"


def call_entry(lib, y, c0, v_plane, out, stream=None, **kw):
    a = dict(ACCEPTED, **kw)
    return lib.kasf_yuv420_to_bgr(y, c0, v_plane if a["c1"] else None, a["layout"], a["n_frames"], a["Hf"], a["Wf"], a["y_row_stride"], a["c_row_stride"],
                                  a["y_frame_stride"], a["c_frame_stride"], out, a["out_row_stride"], a["out_frame_stride"], a["matrix"], 0, 0, stream)


def test_entry_point_refuses_without_touching_a_pointer():
    """Host memory stands in for the device pointers and must come back unchanged; then the same refusals with every pointer null."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    buf = np.full(256, 9, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    for kw, word in REFUSED:
        assert call_entry(lib, p, p, p, p, **kw) == 2 and word in lib.kasf_last_error().decode(), (kw, lib.kasf_last_error())
        assert call_entry(lib, None, None, p, None, **kw) == 2 and word in lib.kasf_last_error().decode(), (kw, lib.kasf_last_error())
    for i, name in enumerate(NULLS):
        ptrs = [p, p, p]
        ptrs[i] = None
        assert call_entry(lib, ptrs[0], ptrs[1], p, ptrs[2]) == 2 and "null pointer" in lib.kasf_last_error().decode(), name
    assert call_entry(lib, None, None, None, None, n_frames=0) == 0, "no frames: nothing to do, nothing to look at"
    assert (buf == 9).all()
