"""The DARK / UDP heatmap decode on the device (kasf_heatmap_decode, K.heatmaps_to_keypoints(decode=...), push_heatmaps(decode=...)) against the numpy restatement
of include/kasf.h's rules (tests/test_heatmap_dark_cpu.py, heatmap_dark_decode_np): equal bits, NaN positions equal.  Shapes are the smallest at which the
kernels take each path: maps of one vector and of several lane passes, maps that are no multiple of 16 bytes (element path), rows that are no multiple of the
vector (the flip test's SPLIT path), map counts that leave a workgroup's last waves without a map (n = 1, 3, 5: 17, 51, 85 maps over workgroups of 4)."""
import functools

import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.test_gpu_heatmap import geometry, same
from tests.test_gpu_heatmap_flip import one_in
from tests.test_heatmap_cpu import F32, GROUPS, fixture, heatmap_decode_np
from tests.test_heatmap_dark_cpu import heatmap_dark_decode_np
from tests.test_heatmap_flip_cpu import merge_np, partner_np

pytestmark = pytest.mark.gpu

TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [(2, 2), (5, 3), (4, 4), (6, 8), (4, 6), (33, 31), (64, 48)]


@functools.lru_cache(maxsize=None)
def peaked_maps(n, H, W, seed=0):
    """[n,17,H,W] float32, every value exact in bfloat16 and float16 (multiples of 1 / 64 below 2): a low random floor with one peak and two raised neighbours
    per map -- the first maps' peaks at the corners, on each edge, at (1,1), (2,2), (H-3,W-3), (H-2,W-2), the two stencils' bounds --, then an all-negative map,
    a constant one, one with a NaN; the rest anywhere.  Shared and never modified."""
    g = np.random.default_rng(seed)
    hm = g.integers(0, 20, (n, 17, H, W)).astype(np.float64) / 64
    flat = hm.reshape(n * 17, H, W)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (1, 1), (2, 2), (H - 3, W - 3), (H - 2, W - 2)]
    spots = [(min(max(y, 0), H - 1), min(max(x, 0), W - 1)) for y, x in spots]
    for i in range(n * 17):
        y, x = spots[i] if i < len(spots) else (int(g.integers(0, H)), int(g.integers(0, W)))
        flat[i, y, x] += 1.0
        if x + 1 < W:
            flat[i, y, x + 1] += 0.625
        if y + 1 < H:
            flat[i, y + 1, x] += 0.375
    k = len(spots)
    flat[k] = -flat[k] - 0.25
    flat[k + 1] = 0.25
    flat[k + 2, H // 2, W // 2] = np.nan
    out = hm.astype(F32)
    assert np.array_equal(torch.from_numpy(out).bfloat16().float().numpy(), out, equal_nan=True)
    out.setflags(write=False)
    return out


def reference(*case):
    """A copy of the cached restatement result of a case (what `same` may wrap in a tensor)."""
    return _reference(*case).copy()


@functools.lru_cache(maxsize=None)
def _reference(n, H, W, decode, kernel, sigma, udp, kind, flip, shift=True, seed=0):
    """The restatement's [n,17,3] for peaked_maps(n, H, W, seed) (merged with peaked_maps(seed + 1) under `flip`) and geometry(n): computed once per case."""
    hm = peaked_maps(n, H, W, seed)
    raw = merge_np(hm, peaked_maps(n, H, W, seed + 1), shift=shift) if flip else hm
    center, scale, boxes = geometry(n, seed=H)
    geo = dict(boxes=boxes, aspect=0.75) if kind == "box" else dict(center=center, scale=scale)
    out = heatmap_dark_decode_np(raw, decode=decode, kernel=kernel, sigma=sigma, udp=udp, **geo)
    out.setflags(write=False)
    return out


def on_device(n, H, W, seed=0) -> torch.Tensor:
    return torch.from_numpy(peaked_maps(n, H, W, seed).copy()).cuda()


def decode_on_device(n, H, W, dtype, decode, kernel=None, sigma=None, udp=None, kind="center_scale", flip=False, shift=True, seed=0, view=lambda t: t, **kw):
    import kasportsformer_amd as K
    hm = view(on_device(n, H, W, seed).to(TORCH[dtype]))
    keep = hm.clone()
    center, scale, boxes = geometry(n, seed=H)
    geo = dict(boxes=boxes, aspect=0.75) if kind == "box" else dict(center=center, scale=scale)
    if flip:
        hmf = view(on_device(n, H, W, seed + 1).to(TORCH[dtype]))
        keep_f = hmf.clone()
        kw.update(flipped=hmf, shift=shift)
    got = K.heatmaps_to_keypoints(hm, decode=decode, kernel=kernel, sigma=sigma, udp=udp, **geo, **kw)
    torch.cuda.synchronize()
    assert same(hm, keep) and (not flip or same(hmf, keep_f)), "inputs are only read"
    return got


CASES = []
for i, (H, W) in enumerate(SHAPES):
    for mi, mode in enumerate(("dark", "dark_udp")):
        CASES.append((H, W, (1, 3, 5)[(i + mi) % 3], ("fp32", "fp16", "bf16")[(i + 2 * mi) % 3], mode, (1, 5, 11, 17)[(i + mi) % 4],
                      ("center_scale", "box")[(i + mi) % 2], (i + mi) % 2 == 1))
CASES += [(3, 1, 3, "fp32", "dark", 5, "box", False), (3, 1, 5, "fp16", "dark_udp", 3, "center_scale", True),     # a side of 1: udp=False only
          (64, 48, 5, "fp32", "dark", 17, "center_scale", False), (64, 48, 1, "fp32", "dark_udp", 11, "box", False)]


@pytest.mark.parametrize("H,W,n,dtype,mode,kernel,kind,flip", CASES)
def test_device_is_the_restatement(H, W, n, dtype, mode, kernel, kind, flip):
    udp = False if min(H, W) < 2 else None
    got = decode_on_device(n, H, W, dtype, mode, kernel=kernel, udp=udp, kind=kind, flip=flip)
    assert tuple(got.shape) == (n, 17, 3) and got.dtype == torch.float32
    assert same(got, reference(n, H, W, mode, kernel, None, udp, kind, flip))


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("mode", ["dark", "dark_udp"])
def test_every_dtype_on_a_vector_map_and_an_element_map(dtype, mode):
    for H, W in ((6, 8), (33, 31)):
        assert same(decode_on_device(3, H, W, dtype, mode, kernel=5), reference(3, H, W, mode, 5, None, None, "center_scale", False))
        assert same(decode_on_device(3, H, W, dtype, mode, kernel=5, flip=True), reference(3, H, W, mode, 5, None, None, "center_scale", True))


@pytest.mark.parametrize("mode,udp", [("dark", True), ("dark_udp", False), ("quarter", True)])
def test_udp_is_independent_of_the_step(mode, udp):
    got = decode_on_device(3, 6, 8, "fp32", mode, udp=udp, kernel=None if mode == "quarter" else 5)
    assert same(got, reference(3, 6, 8, mode, None if mode == "quarter" else 5, None, udp, "center_scale", False))
    assert not same(got, reference(3, 6, 8, mode, None if mode == "quarter" else 5, None, not udp, "center_scale", False))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_a_view_one_element_off_the_16_byte_grid_takes_the_element_path_to_the_same_answer(dtype, flip):
    got = decode_on_device(3, 6, 8, dtype, "dark_udp", kernel=11, flip=flip, view=one_in)
    assert same(got, reference(3, 6, 8, "dark_udp", 11, None, None, "center_scale", flip))


def test_an_explicit_sigma_and_the_default_kernel():
    assert same(decode_on_device(1, 33, 31, "fp32", "dark", kernel=7, sigma=1.25), reference(1, 33, 31, "dark", 7, 1.25, None, "center_scale", False))
    assert same(decode_on_device(1, 33, 31, "fp32", "dark"), reference(1, 33, 31, "dark", 11, None, None, "center_scale", False))
    assert not same(decode_on_device(1, 33, 31, "fp32", "dark", kernel=7), reference(1, 33, 31, "dark", 7, 1.25, None, "center_scale", False))


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("H,W,dtype", [(6, 8, "fp32"), (4, 6, "fp32"), (33, 31, "fp16"), (8, 12, "fp16")])
def test_the_flip_test_with_and_without_shift_and_its_merged_maps(H, W, dtype, shift):
    """ROW (6 x 8 fp32), SPLIT (4 x 6 fp32, 8 x 12 fp16) and ELEM (33 x 31) under both modes; merged=True returns merge_np's maps."""
    for mode in ("dark", "dark_udp"):
        got = decode_on_device(3, H, W, dtype, mode, kernel=5, flip=True, shift=shift, merged=True)
        assert same(got.keypoints, reference(3, H, W, mode, 5, None, None, "center_scale", True, shift))
        assert same(got.merged, merge_np(peaked_maps(3, H, W, 0), peaked_maps(3, H, W, 1), shift=shift))
        assert not same(got.keypoints, reference(3, H, W, mode, 5, None, None, "center_scale", False))


def test_custom_pairs_reach_the_new_entry():
    import kasportsformer_amd as K
    hm, hmf = (on_device(1, 6, 8, s) for s in (0, 1))
    center, scale, _ = geometry(1, seed=6)
    got = K.heatmaps_to_keypoints(hm, center, scale, flipped=hmf, pairs=[(0, 16), (3, 4)], decode="dark", kernel=3)
    raw = merge_np(peaked_maps(1, 6, 8, 0), peaked_maps(1, 6, 8, 1), partner=partner_np(((0, 16), (3, 4))))
    assert same(got, heatmap_dark_decode_np(raw, center, scale, decode="dark", kernel=3))


def test_h36m_layout_is_coco_to_h36m_of_the_coco_result():
    import kasportsformer_amd as K
    coco = decode_on_device(3, 6, 8, "fp32", "dark_udp", kernel=5)
    h36m = decode_on_device(3, 6, 8, "fp32", "dark_udp", kernel=5, layout="h36m")
    assert same(h36m, K.coco_to_h36m(coco)) and not same(h36m, coco)


def test_the_same_bits_again_and_no_persons_is_no_work():
    import kasportsformer_amd as K
    a, b = (decode_on_device(5, 33, 31, "bf16", "dark", kernel=11, flip=True) for _ in range(2))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for mode in ("dark", "dark_udp"):
        out = K.heatmaps_to_keypoints(torch.zeros((0, 17, 6, 8), device="cuda"), torch.zeros((0, 2)), torch.zeros((0, 2)), decode=mode)
        assert tuple(out.shape) == (0, 17, 3) and out.is_cuda
    res = K.heatmaps_to_keypoints(torch.zeros((0, 17, 6, 8), device="cuda"), torch.zeros((0, 2)), torch.zeros((0, 2)), decode="dark",
                                  flipped=torch.zeros((0, 17, 6, 8), device="cuda"), merged=True)
    assert tuple(res.keypoints.shape) == (0, 17, 3) and tuple(res.merged.shape) == (0, 17, 6, 8)


@pytest.mark.parametrize("group", GROUPS)
def test_defaults_are_the_existing_decode_bit_for_bit(group):
    """All new arguments at their defaults, spelled out: the existing restatement on the fixture the reference's own get_final_preds wrote."""
    import kasportsformer_amd as K
    fx = fixture()
    hm, center, scale = fx[group + "_hm"], fx[group + "_center"], fx[group + "_scale"]
    got = K.heatmaps_to_keypoints(torch.from_numpy(hm).cuda(), center, scale, decode="quarter", kernel=None, sigma=None, udp=None)
    assert same(got, heatmap_decode_np(hm, center, scale)) and same(got, K.heatmaps_to_keypoints(torch.from_numpy(hm).cuda(), center, scale))
    assert same(K.heatmaps_to_keypoints(torch.from_numpy(hm).cuda(), center, scale, udp=False), got)


def test_entry_point_refuses_device_pointers_too():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    hm, hmf, geom = torch.ones(17 * 15, device="cuda"), torch.ones(17 * 15, device="cuda"), torch.ones(4, device="cuda")
    out = torch.full((51,), 7.0, device="cuda")
    w = np.full(3, 0.25, F32)
    wp = w.ctypes.data
    f = lib.kasf_heatmap_decode
    for args in ((ptr(hm), None, 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 3, wp, 3, 0, 0, ptr(out), None, None),
                 (ptr(hm), None, 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, wp, 4, 0, 0, ptr(out), None, None),
                 (ptr(hm), None, 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, None, 3, 0, 0, ptr(out), None, None),
                 (ptr(hm), None, 0, 1, 15, 1, None, 1, ptr(geom), 0, 1.0, 2, wp, 3, 1, 0, ptr(out), None, None),
                 (ptr(hm), ptr(hmf), 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, wp, 3, 0, 0, ptr(out), None, ptr(hmf)),
                 (ptr(hm), None, 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, wp, 3, 0, 1, ptr(out), None, None)):
        assert f(*args, stream()) == 2 and lib.kasf_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((hm == 1).all()) and bool((hmf == 1).all())


def test_stream_push_heatmaps_is_push_of_the_decoded_keypoints():
    import kasportsformer_amd as K
    m = make_pair(1, 27, "fp32")[1].eval()
    S, H, W = 3, 16, 12
    a, b = (K.StreamLifter(m, 1920, 1080, slots=S, layout="coco") for _ in range(2))
    center, scale, boxes = geometry(S, seed=9)
    for tick, kw in enumerate((dict(decode="dark_udp"), dict(decode="dark", kernel=5), dict(decode="dark_udp", kernel=3, sigma=0.9, udp=False), dict(udp=True))):
        hm, hmf = (on_device(S, H, W, 20 + tick + s) for s in (0, 1))
        if tick % 2:
            kw = dict(kw, flipped=hmf, shift=False)
        got = a.push_heatmaps(hm, center, scale, **kw)
        kp = K.heatmaps_to_keypoints(hm, center, scale, **kw)
        assert not torch.equal(kp, K.heatmaps_to_keypoints(hm, center, scale, **{k: v for k, v in kw.items() if k in ("flipped", "shift")}))
        assert same(got, b.push(kp)), tick
    assert same(a._ring, b._ring)                               # the NaN map's NaN score sits in both rings
    with pytest.raises(ValueError):
        a.push_heatmaps(hm, center, scale, decode="dark", kernel=4)
    assert np.array_equal(a.counts, b.counts), "a refused call leaves the state as it was"


def test_tracked_push_heatmaps_is_push_of_the_decoded_keypoints():
    import kasportsformer_amd as K
    from tests.test_gpu_tracked import B, _dev, _lifter
    from tests.tracked_ref import script
    T, R = 27, 2
    n = B * R
    pushed, decoded = _lifter(), _lifter()
    center = torch.tensor([[600.0, 350.0]] * n, device="cuda") + torch.arange(n, device="cuda")[:, None]
    scale = torch.tensor([[1.5, 2.0]] * n, device="cuda")
    for tick, arrays in enumerate(script(T, 8)[5:8]):
        t = _dev(arrays)
        hm = on_device(n, 16, 12, 40 + tick)
        kw = (dict(decode="dark_udp"), dict(decode="dark", kernel=7), dict(decode="dark_udp", kernel=5, udp=False))[tick]
        got = pushed.push_heatmaps(hm, center, scale, t, **kw)
        want = decoded.push(K.heatmaps_to_keypoints(hm, center, scale, layout="h36m", **kw), t)
        assert all(same(u, v) if u.is_floating_point() else torch.equal(u, v) for u, v in zip(got, want)), tick      # the NaN map's joint is NaN in both
        assert want.valid.any() and want.poses.nan_to_num().abs().sum() > 0
    with pytest.raises(ValueError):
        pushed.push_heatmaps(hm, center, scale, t, decode="dark", refine=False)
