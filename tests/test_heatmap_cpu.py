"""Host side of the heatmap decode (kasportsformer_amd.heatmaps_to_keypoints / StreamLifter.push_heatmaps, kasf_heatmap_keypoints): the numpy restatement
the GPU tests hold the kernel to (tests/test_gpu_heatmap.py imports it from here), tied to the fixture the reference's own get_final_preds, get_max_preds and
box_to_center_scale wrote (tests/golden/make_heatmap_golden.py); the refusals of the entry point and of the Python surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = np.float32, np.float64
GROUPS = ("a", "b")                                             # fixture groups: a = 96 x 72 maps, b = 64 x 48 maps


def fixture():
    return np.load(os.path.join(GOLDEN, "heatmap_decode.npz"), allow_pickle=False)


def box_to_center_scale_np(boxes, aspect):
    """box_to_center_scale (demo/lib/hrnet/lib/utils/utilitys.py:102-135) on float32 boxes [...,4] = x1, y1, x2, y2: fp64 arithmetic on the widened box, the
    box grown to width / height = aspect, / 200, stored as fp32, then * 1.25 in fp32 unless center x == -1 -> (center [...,2], scale [...,2]) float32."""
    b = np.asarray(boxes, dtype=F32).astype(F64)
    a = F64(aspect)
    x1, y1, x2, y2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    bw, bh = x2 - x1, y2 - y1
    center = np.stack((x1 + bw * 0.5, y1 + bh * 0.5), axis=-1).astype(F32)
    wide = bw > a * bh
    tall = ~wide & (bw < a * bh)
    bh2, bw2 = np.where(wide, bw * 1.0 / a, bh), np.where(tall, bh * a, bw)
    scale = np.stack((bw2 * 1.0 / 200, bh2 * 1.0 / 200), axis=-1).astype(F32)
    scale = np.where((center[..., :1] != -1), scale * F32(1.25), scale)
    assert center.dtype == scale.dtype == F32
    return center, scale


def heatmap_decode_np(hm, center=None, scale=None, *, boxes=None, aspect=None, refine=True, parts=False):
    """get_final_preds (demo/lib/hrnet/lib/utils/inference.py:21-82) on hm [n,17,H,W] (float32, or float16 widened exactly), restated with the operations and
    precisions of include/kasf.h's kasf_heatmap_keypoints: np.argmax's first maximum / first NaN, the score = the value there, (0, 0) where "score > 0" is false,
    the strict-bounds quarter-pixel step in fp32, the three fp32 anchors of transform_preds and its affine in closed form in fp64, rounded once.
    -> [n,17,3] float32 image x, y, score; with parts=True also the argmax positions and the refined heatmap coordinates, [n,17,2] float32 each."""
    h = np.asarray(hm)
    h = h if h.dtype == F32 else h.astype(F32)
    n, J, H, W = h.shape
    if boxes is not None:
        center, scale = box_to_center_scale_np(boxes, aspect)
    center, scale = np.asarray(center, dtype=F32).reshape(n, 2), np.asarray(scale, dtype=F32).reshape(n, 2)
    flat = h.reshape(n, J, H * W)
    idx = np.argmax(flat, axis=2) if H * W else np.zeros((n, J), np.int64)
    score = np.take_along_axis(flat, idx[..., None], axis=2)[..., 0]
    with np.errstate(invalid="ignore"):
        found = score > 0
    px, py = np.where(found, idx % W, 0), np.where(found, idx // W, 0)
    pos = np.stack((px, py), axis=-1).astype(F32)
    coords = pos.copy()
    if refine:
        inside = (1 < px) & (px < W - 1) & (1 < py) & (py < H - 1)
        with np.errstate(invalid="ignore"):
            for i, j in np.argwhere(inside):
                m, x, y = h[i, j], px[i, j], py[i, j]
                coords[i, j, 0] += np.sign(m[y, x + 1] - m[y, x - 1]) * F32(0.25)
                coords[i, j, 1] += np.sign(m[y + 1, x] - m[y - 1, x]) * F32(0.25)
    assert coords.dtype == F32
    cx, cy = center[:, 0], center[:, 1]
    with np.errstate(all="ignore"):
        sw = scale[:, 0] * F32(200)
        s1y = (cy.astype(F64) + (sw * F32(-0.5)).astype(F64)).astype(F32)
        dy = cy - s1y
        s2x = cx + (-dy)
        assert sw.dtype == dy.dtype == s2x.dtype == F32
        half_w, half_h = F64(W) * 0.5, F64(H) * 0.5
        kx = (cx.astype(F64) - s2x.astype(F64)) / half_w
        ky = (cy.astype(F64) - s1y.astype(F64)) / half_w
        out = np.empty((n, J, 3), F32)
        out[..., 0] = cx.astype(F64)[:, None] + (coords[..., 0].astype(F64) - half_w) * kx[:, None]
        out[..., 1] = cy.astype(F64)[:, None] + (coords[..., 1].astype(F64) - half_h) * ky[:, None]
    out[..., 2] = score
    return (out, pos, coords) if parts else out


def ulp_distance(a, b):
    """Distance in representable float32 values between finite float32 arrays."""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fixture_loads_without_pickles_and_is_small():
    path = os.path.join(GOLDEN, "heatmap_decode.npz")
    assert os.path.getsize(path) < 1024 * 1024
    fx = fixture()
    for g, (H, W) in zip(GROUPS, ((96, 72), (64, 48))):
        hm = fx[g + "_hm"]
        P = hm.shape[0]
        assert hm.dtype == np.float16 and hm.shape == (P, 17, H, W) and P >= 4
        assert fx[g + "_center"].shape == fx[g + "_scale"].shape == (P, 2) and fx[g + "_boxes"].shape == (P, 4)
        assert fx[g + "_aspect"].dtype == F64 and fx[g + "_aspect"].shape == ()
        assert fx[g + "_maxvals"].shape == (P, 17, 1) and fx[g + "_maxpos"].shape == (P, 17, 2)
        for r in (0, 1):
            for name in ("coords", "preds_cs", "preds_box"):
                assert fx[f"{g}_{name}_r{r}"].shape == (P, 17, 2) and fx[f"{g}_{name}_r{r}"].dtype == F32
        assert (fx[g + "_box_center"][:, 0] == -1).sum() == 1, "one box whose center x is -1 (no 1.25)"
    assert fx["a_center"].max() < 1000 and fx["b_center"].max() > 6000, "frames from a few hundred to 8,000 px"
    e = fx["a_hm"][-1].astype(F32)                              # the hand-made person: ties, all-zero, all-negative
    assert (e[0] == e[0].max()).sum() == 2 and (e[14] == e[14].max()).sum() == 3 and not e[1].any() and e[2].max() < 0


def test_restatement_is_the_reference_on_the_fixture():
    """Argmax positions, maxvals and refined heatmap coordinates bit for bit; image-space preds within 1 fp32 ulp (both sides round one fp64 value that
    differs by the error of the shim's float64 solve, ~1e-13 relative), and no more coordinates off than the generator counted: 1 of the 2 groups x 2 x 2 x
    85 x 2 = 1,360 coordinates is 1 ulp off, the rest are bit-identical (heatmap_decode.npz: neq_count = 1, max_ulp = 1)."""
    fx = fixture()
    neq, worst = 0, 0
    for g in GROUPS:
        hm = fx[g + "_hm"]
        for r in (0, 1):
            out, pos, coords = heatmap_decode_np(hm, fx[g + "_center"], fx[g + "_scale"], refine=bool(r), parts=True)
            assert same_bits(pos, fx[g + "_maxpos"])
            assert same_bits(out[..., 2], fx[g + "_maxvals"][..., 0])
            assert same_bits(coords, fx[f"{g}_coords_r{r}"])
            box = heatmap_decode_np(hm, boxes=fx[g + "_boxes"], aspect=fx[g + "_aspect"], refine=bool(r))
            for mine, ref in ((out[..., :2], fx[f"{g}_preds_cs_r{r}"]), (box[..., :2], fx[f"{g}_preds_box_r{r}"])):
                d = ulp_distance(mine, ref)
                neq, worst = neq + int((d != 0).sum()), max(worst, int(d.max()))
    print(f"restatement vs reference: {neq} coordinates not bit-equal (recorded {int(fx['neq_count'])}), largest distance {worst} ulp")
    assert worst <= 1
    assert neq <= int(fx["neq_count"]) and int(fx["max_ulp"]) <= 1


def test_refinement_took_every_branch_on_the_fixture():
    fx = fixture()
    step = fx["a_coords_r1"][-1] - fx["a_maxpos"][-1]           # the hand-made person, maps as make_heatmap_golden.edge_person lays them out
    W, H = 72, 96
    assert tuple(fx["a_maxpos"][-1][0]) == (20, 7) and tuple(step[0]) == (0.25, -0.25), "two equal maxima: the first in row-major order, refined there"
    assert tuple(fx["a_maxpos"][-1][14]) == (9, 20), "three equal maxima"
    assert not fx["a_maxpos"][-1][[1, 2]].any() and not step[[1, 2]].any(), "all-zero and all-negative maps: (0, 0), never refined"
    for j, px in zip((3, 4, 5, 6), (0, 1, W - 2, W - 1)):          # 1 < px < W - 1: px = 1 is not refined, px = W - 2 is
        assert fx["a_maxpos"][-1][j, 0] == px and tuple(step[j]) == ((0.25, 0.25) if px == W - 2 else (0, 0)), (j, px, step[j])
    for j, py in zip((7, 8, 9, 10), (0, 1, H - 2, H - 1)):
        assert fx["a_maxpos"][-1][j, 1] == py and tuple(step[j]) == ((0.25, 0.25) if py == H - 2 else (0, 0)), (j, py, step[j])
    assert step[11, 0] == 0 and step[11, 1] != 0 and step[12, 0] != 0 and step[12, 1] == 0, "equal neighbours on one axis: sign(0) = 0"
    assert step[13, 0] == -0.25 and abs(step[15]).max() == 0.25 and abs(step[16]).max() == 0.25, "px = 2 and px = W - 3 are refined"
    assert tuple(step[15]) == (0.25, -0.25) and tuple(step[16]) == (-0.25, 0.25)
    assert np.array_equal(fx["a_coords_r0"], fx["a_maxpos"])


def test_box_path_gives_the_reference_center_and_scale_bit_for_bit():
    fx = fixture()
    for g in GROUPS:
        c, s = box_to_center_scale_np(fx[g + "_boxes"], fx[g + "_aspect"])
        assert same_bits(c, fx[g + "_box_center"]) and same_bits(s, fx[g + "_box_scale"])
        assert not np.array_equal(s[:, 0] * F32(200), (fx[g + "_boxes"][:, 2] - fx[g + "_boxes"][:, 0]) * F32(1.25)), "some boxes were widened"


def test_nan_maps_follow_numpy_argmax_and_amax():
    g = np.random.default_rng(5)
    hm = g.uniform(-1, 1, size=(2, 17, 9, 7)).astype(F32)
    hm[0, 3, 4, 2] = np.nan                                     # one NaN
    hm[0, 5, 6, 1] = hm[0, 5, 2, 5] = np.nan                    # two: the first one counts
    hm[1, 0, 0, 0] = np.nan
    hm[1, 16, 8, 6] = np.nan
    center, scale = np.array([[300, 200], [50, 60]], F32), np.array([[1.5, 2], [0.7, 0.9]], F32)
    out, pos, coords = heatmap_decode_np(hm, center, scale, parts=True)
    flat = hm.reshape(2, 17, -1)
    with np.errstate(invalid="ignore"):
        amax, arg = np.amax(flat, axis=2), np.argmax(flat, axis=2)
    nan = np.isnan(amax)
    assert nan.sum() == 4 and np.array_equal(np.isnan(out[..., 2]), nan) and np.array_equal(out[..., 2][~nan], amax[~nan])
    assert arg[0, 3] == 4 * 7 + 2 and arg[0, 5] == 2 * 7 + 5 and arg[1, 0] == 0 and arg[1, 16] == 62
    assert not pos[nan].any() and not coords[nan].any(), "a NaN score is not > 0: the position is (0, 0), unrefined"
    assert np.isfinite(out[..., :2]).all()
    clean = np.where(np.isnan(hm), F32(-2), hm)
    keep = ~nan
    assert same_bits(out[keep], heatmap_decode_np(clean, center, scale)[keep]), "a NaN map leaves the other maps alone"
    hm2 = hm.copy()
    hm2[1, 2] = 0
    hm2[1, 2, 4, 3], hm2[1, 2, 4, 2], hm2[1, 2, 4, 4] = 1, -np.inf, -np.inf      # -inf - -inf: the difference, its sign and x are NaN; the score is not
    out2 = heatmap_decode_np(hm2, center, scale)
    assert out2[1, 2, 2] == 1 and np.isnan(out2[1, 2, 0]) and np.isfinite(out2[1, 2, 1])


def test_sixteen_bit_inputs_are_widened_exactly():
    fx = fixture()
    hm16 = fx["b_hm"]
    assert same_bits(heatmap_decode_np(hm16, fx["b_center"], fx["b_scale"]), heatmap_decode_np(hm16.astype(F32), fx["b_center"], fx["b_scale"]))
    assert np.array_equal(hm16.astype(F32).astype(np.float16), hm16)


def test_entry_point_refuses_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    assert "kasf_heatmap_keypoints" in _lib.SIGNATURES and hasattr(lib, "kasf_heatmap_keypoints")
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "kasf.h")).read()
    assert "int kasf_heatmap_keypoints(const void* hm, int32_t dtype, int64_t n, int32_t H, int32_t W," in hdr and "ADDED under ABI 12" in hdr
    assert _lib.ABI_VERSION == lib.kasf_version() == 12
    hm, geom, out, tmp = np.full(17 * 15, 3, F32), np.full(4, 5, F32), np.full(51, 7, F32), np.full(51, 9, F32)
    p = [a.ctypes.data_as(C.c_void_p) for a in (hm, geom, out, tmp)]
    f = lib.kasf_heatmap_keypoints      # (hm, dtype, n, H, W, geom, geom_kind, aspect, refine, out_layout, out, coco_scratch, stream)

    def call(hm=p[0], dtype=0, n=1, H=5, W=3, geom=p[1], kind=0, aspect=1.0, refine=1, layout=0, out=p[2], tmp=p[3]):
        return f(hm, dtype, n, H, W, geom, kind, aspect, refine, layout, out, tmp, None)

    assert call(n=0) == 0 and call(None, n=0, geom=None, out=None, tmp=None) == 0          # nothing to do
    refused = [dict(n=-1), dict(H=0), dict(W=0), dict(H=-5), dict(H=4097, W=4096), dict(H=1 << 30, W=1 << 30), dict(dtype=3), dict(dtype=-1),
               dict(kind=2), dict(kind=-1), dict(layout=2), dict(layout=-1), dict(kind=1, aspect=0.0), dict(kind=1, aspect=-0.5),
               dict(kind=1, aspect=float("nan")), dict(hm=None), dict(geom=None), dict(out=None), dict(layout=1, tmp=None)]
    for kw in refused:
        assert call(**kw) == 2, kw
        assert lib.kasf_last_error(), kw
    assert (hm == 3).all() and (geom == 5).all() and (out == 7).all() and (tmp == 9).all(), "a refused call touches no buffer"


def test_python_surface_refuses_before_any_launch():
    import kasportsformer_amd as K
    assert "heatmaps_to_keypoints" in K.__all__ and "heatmaps_to_keypoints" in K.__doc__
    hm = np.zeros((2, 17, 5, 3), F32)
    c, s, b = np.zeros((2, 2), F32), np.ones((2, 2), F32), np.array([[0, 0, 4, 4]] * 2, F32)
    with pytest.raises(RuntimeError):
        K.heatmaps_to_keypoints(hm, c, s, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.heatmaps_to_keypoints(hm, c, s)
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.heatmaps_to_keypoints(torch.zeros((17, 4, 4), dtype=torch.bfloat16), boxes=torch.zeros(4), aspect=0.5, layout="h36m")
    h = K.heatmaps_to_keypoints
    for exc, call in ((TypeError, lambda: h(hm.astype(F64), c, s)),
                      (TypeError, lambda: h(hm.tolist(), c, s)),
                      (TypeError, lambda: h(torch.zeros((2, 17, 5, 3), dtype=torch.int32), c, s)),
                      (TypeError, lambda: h(hm, c.astype(F64), s)),
                      (TypeError, lambda: h(hm, boxes=b.astype(np.float16), aspect=1.0)),
                      (ValueError, lambda: h(hm[:, :16], c, s)),
                      (ValueError, lambda: h(hm[0, 0], c, s)),
                      (ValueError, lambda: h(hm[:, :, :0], c, s)),
                      (ValueError, lambda: h(hm)),
                      (ValueError, lambda: h(hm, c)),
                      (ValueError, lambda: h(hm, c, s[:1])),
                      (ValueError, lambda: h(hm, c, s, boxes=b, aspect=1.0)),
                      (ValueError, lambda: h(hm, c, s, aspect=1.0)),
                      (ValueError, lambda: h(hm, boxes=b)),
                      (ValueError, lambda: h(hm, boxes=b, aspect=0.0)),
                      (ValueError, lambda: h(hm, boxes=b, aspect=float("inf"))),
                      (ValueError, lambda: h(hm, boxes=b[:, :3], aspect=1.0)),
                      (ValueError, lambda: h(hm, c, s, layout="COCO")),
                      (ValueError, lambda: h(hm, c, s, layout=None))):
        with pytest.raises(exc):
            call()
    assert not hm.any() and not c.any()


def test_push_heatmaps_exists_and_needs_a_gpu():
    import kasportsformer_amd as K
    assert callable(K.StreamLifter.push_heatmaps)
    m = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=27, compute_dtype="fp32")
    with pytest.raises(RuntimeError):
        K.StreamLifter(m, 1280, 720, slots=2)
