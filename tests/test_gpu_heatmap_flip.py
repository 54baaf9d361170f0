"""The flip-tested heatmap decode on the device (kasf_heatmap_flip_keypoints, K.heatmaps_to_keypoints(flipped=...), push_heatmaps(flipped=...)) against the
numpy restatement of tests/test_heatmap_flip_cpu.py, which that file ties to the reference's own outputs.  Device and restatement perform the same IEEE
operations, so every comparison is exact (torch.equal; where a NaN is expected, equal NaN positions and equal values elsewhere).  Nothing here provokes a
fault: refusals are tested through the error code.

The kernel's mapping (k_heatmap_flip_keypoints in csrc/k_heatmap.hip), which the tie tests place their maxima by: one wavefront per merged map; the DIRECT map is read as vectors of
VW values (16 bytes: VW = 4 for fp32, 8 for fp16 / bf16; VW = 1 on the element-wise path, taken when either array does not start on a 16-byte boundary or a map
is not a multiple of 16 bytes); vector v is read by lane v % 64 in that lane's pass v // 64, and value k of it is merged map index v * VW + k = row y, column
x + k.  Its flipped operand is element y * W + src_x(x + k) of the partner map: when W is a multiple of VW, slot VW - 1 - k (no shift) or VW - k (shift) of the
aligned vector at columns W - x - VW .. W - x - 1 of row y, with slot "VW" = one element load of column min(W - x, W - 1); otherwise element loads."""
import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.test_gpu_heatmap import geometry, index_of, random_maps, same
from tests.test_heatmap_cpu import F32, GROUPS
from tests.test_heatmap_flip_cpu import COCO_PAIRS, fixture, heatmap_flip_decode_np, merge_np, partner_np, src_x_np

pytestmark = pytest.mark.gpu

_FIXTURE = {}


def golden():
    if not _FIXTURE:
        fx = fixture()
        _FIXTURE.update({k: fx[k] for k in fx.files})
    return _FIXTURE


def pair_of_maps(n, H, W, seed):
    """Two independent arrays of random maps: direct and flipped."""
    return random_maps(n, H, W, seed=seed), random_maps(n, H, W, seed=seed + 5000)


def one_in(t: torch.Tensor) -> torch.Tensor:
    """The same values in a contiguous view that starts one element into a larger allocation (not 16-byte aligned)."""
    store = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    store[1:] = t.reshape(-1)
    view = store[1:].view(t.shape)
    assert view.data_ptr() % 16 == t.element_size() and view.is_contiguous()
    return view


@pytest.mark.parametrize("kind", ["center_scale", "box"])
@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_fixture_decodes_to_the_restatement(group, refine, shift, kind):
    """Both map sizes, refine and shift on and off, both geometry kinds: blobs, and the hand-made person in which the merge decides every outcome
    (tests/golden/make_heatmap_flip_golden.py).  With shift the merged maps are the reference's recorded ones bit for bit."""
    import kasportsformer_amd as K
    fx = golden()
    hm, hmf = torch.from_numpy(fx[group + "_hm"]).cuda(), torch.from_numpy(fx[group + "_hmf"]).cuda()
    keep = hm.clone(), hmf.clone()
    if kind == "box":
        kw = dict(boxes=geometry(hm.shape[0], seed=3)[2], aspect=1080 / 1920)
    else:
        kw = dict(center=fx[group + "_center"], scale=fx[group + "_scale"])
    got = K.heatmaps_to_keypoints(hm, refine=refine, flipped=hmf, shift=shift, merged=True, **kw)
    assert isinstance(got, tuple) and got._fields == ("keypoints", "merged")
    assert got.keypoints.is_cuda and got.keypoints.dtype == torch.float32 and tuple(got.keypoints.shape) == (hm.shape[0], 17, 3)
    want = heatmap_flip_decode_np(fx[group + "_hm"], fx[group + "_hmf"], refine=refine, shift=shift, **kw)
    assert torch.equal(got.keypoints.cpu(), torch.from_numpy(want))
    assert got.merged.dtype == torch.float32 and torch.equal(got.merged.cpu(), torch.from_numpy(merge_np(fx[group + "_hm"], fx[group + "_hmf"], shift=shift)))
    if shift:
        assert torch.equal(got.merged.cpu(), torch.from_numpy(fx[group + "_merged"]))
        assert torch.equal(got.keypoints[..., 2].cpu(), torch.from_numpy(fx[group + "_maxvals"][..., 0]))
    assert torch.equal(hm, keep[0]) and torch.equal(hmf, keep[1]), "the heatmaps are only read"


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("H,W", [(5, 3), (7, 5), (4, 4), (6, 8), (3, 1), (2, 2), (33, 31), (64, 48), (96, 72)])
def test_map_shapes_and_map_count_tails(H, W, n):
    """W = 1 and W = 2, the smallest maps where src_x can go wrong; 5 x 3, 7 x 5, 3 x 1, 2 x 2, 33 x 31 on the element-wise path; 4 x 4 and 6 x 8 on the vector
    path with idle lanes and, with shift, flipped segments that straddle row ends; the two network sizes; 17, 51, 85 maps is never a multiple of the 4 maps
    of a workgroup.  fp32 and fp16 take different paths at the same shape (6 x 8: rows of two fp32 vectors, one fp16 vector)."""
    import kasportsformer_amd as K
    hm, hmf = pair_of_maps(n, H, W, seed=H * 100 + n)
    center, scale, boxes = geometry(n, seed=n)
    dev = [torch.from_numpy(a).cuda() for a in (hm, hmf, center, scale)]
    for shift in (True, False):
        for refine in (True, False):
            got = K.heatmaps_to_keypoints(dev[0], dev[2], dev[3], refine=refine, flipped=dev[1], shift=shift)
            assert torch.equal(got.cpu(), torch.from_numpy(heatmap_flip_decode_np(hm, hmf, center, scale, refine=refine, shift=shift))), (shift, refine)
        got = K.heatmaps_to_keypoints(dev[0], boxes=torch.from_numpy(boxes).cuda(), aspect=1080 / 1920, flipped=dev[1], shift=shift, merged=True)
        assert torch.equal(got.keypoints.cpu(), torch.from_numpy(heatmap_flip_decode_np(hm, hmf, boxes=boxes, aspect=1080 / 1920, shift=shift)))
        assert torch.equal(got.merged.cpu(), torch.from_numpy(merge_np(hm, hmf, shift=shift)))
        h16, f16 = dev[0].half(), dev[1].half()
        got = K.heatmaps_to_keypoints(h16, dev[2], dev[3], flipped=f16, shift=shift)
        assert torch.equal(got.cpu(), torch.from_numpy(heatmap_flip_decode_np(h16.cpu(), f16.cpu(), center, scale, shift=shift)))
    assert torch.equal(dev[0].cpu(), torch.from_numpy(hm)) and torch.equal(dev[1].cpu(), torch.from_numpy(hmf))


def test_rows_that_are_no_multiple_of_the_vector_keep_the_direct_operand_on_vectors():
    """4 x 6 fp32 and 8 x 12 fp16: a map is a multiple of 16 bytes, a row is not -- vectors straddle row ends on both sides."""
    import kasportsformer_amd as K
    for (H, W), dtype in (((4, 6), torch.float32), ((8, 12), torch.float16), ((8, 12), torch.bfloat16)):
        hm, hmf = (torch.from_numpy(a).cuda().to(dtype) for a in pair_of_maps(3, H, W, seed=77))
        center, scale, _ = geometry(3, seed=78)
        for shift in (True, False):
            got = K.heatmaps_to_keypoints(hm, center, scale, flipped=hmf, shift=shift, merged=True)
            assert torch.equal(got.keypoints.cpu(), torch.from_numpy(heatmap_flip_decode_np(hm.cpu(), hmf.cpu(), center, scale, shift=shift)))
            assert torch.equal(got.merged.cpu(), torch.from_numpy(merge_np(hm.cpu(), hmf.cpu(), shift=shift)))


def test_no_persons_is_no_work():
    import kasportsformer_amd as K
    from kasportsformer_amd import _lib
    z = torch.zeros((0, 17, 5, 3), device="cuda")
    empty = K.heatmaps_to_keypoints(z, torch.zeros((0, 2)), torch.zeros((0, 2)), flipped=z.clone(), merged=True)
    assert tuple(empty.keypoints.shape) == (0, 17, 3) and tuple(empty.merged.shape) == (0, 17, 5, 3) and empty.merged.is_cuda
    out = torch.full((51,), 7.0, device="cuda")
    hm, geom = torch.zeros(17 * 15, device="cuda"), torch.ones(4, device="cuda")
    assert _lib.load().kasf_heatmap_flip_keypoints(ptr(hm), ptr(hm), 0, 0, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, 1, ptr(out), ptr(out), None, stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "n = 0 leaves the output alone"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("which", ["direct", "flipped", "both"])
def test_a_misaligned_operand_takes_the_elementwise_path_to_the_same_answer(which, dtype):
    import kasportsformer_amd as K
    n, H, W = 3, 64, 48
    hm, hmf = (torch.from_numpy(a).cuda().to(dtype) for a in pair_of_maps(n, H, W, seed=31))
    a = one_in(hm) if which in ("direct", "both") else hm
    b = one_in(hmf) if which in ("flipped", "both") else hmf
    assert hm.data_ptr() % 16 == 0 and hmf.data_ptr() % 16 == 0
    center, scale, _ = geometry(n, seed=32)
    for shift in (True, False):
        got = K.heatmaps_to_keypoints(a, center, scale, flipped=b, shift=shift, merged=True)
        aligned = K.heatmaps_to_keypoints(hm, center, scale, flipped=hmf, shift=shift, merged=True)
        assert torch.equal(got.keypoints, aligned.keypoints) and torch.equal(got.merged, aligned.merged)
        assert torch.equal(got.keypoints.cpu(), torch.from_numpy(heatmap_flip_decode_np(hm.cpu(), hmf.cpu(), center, scale, shift=shift)))
    assert torch.equal(a, hm) and torch.equal(b, hmf)


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("path", ["fp32", "fp16", "bf16", "elementwise"])
def test_equal_merged_maxima_go_to_the_first_in_row_major_order(path, shift):
    """Two and three equal MERGED maxima placed by the kernel's mapping (module docstring), as tests/test_gpu_heatmap.py places them, each made by another
    operand in turn: by the direct one (1.5 + 0), by the flipped one (0 + 1.5), by both (0.75 + 0.75) -- (a + b) * 0.5 = 0.75 exactly each time."""
    import kasportsformer_amd as K
    H, W = 64, 48
    vw = {"fp32": 4, "fp16": 8, "bf16": 8, "elementwise": 1}[path]
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(path, torch.float32)
    last = 3072 // (64 * vw) - 1
    first = index_of(50, 1, 1, vw)
    cases = {
        0: [first, index_of(10, 3, max(vw - 2, 0), vw)],
        1: [first, index_of(10, 3, max(vw - 2, 0), vw), index_of(10, last, 0, vw)],
        2: [index_of(7, 2, 0, vw), index_of(7, last, vw - 1, vw)],
        3: [index_of(63, 0, vw - 1, vw), index_of(0, 1, 0, vw)],
        4: [index_of(0, last, 0, vw), index_of(63, last, vw - 1, vw)],
        5: [index_of(31, 2, 0, vw), index_of(32, 2, 0, vw)],
        8: [index_of(3, 1, 0, vw), index_of(3, 1, 1, vw) if vw > 1 else index_of(4, 1, 0, vw)],      # slot 0 (the shifted path's element load) against its neighbour
    }
    if vw > 1:
        cases[6] = [index_of(20, 2, 1, vw), index_of(20, 2, 3, vw)]
        cases[7] = [index_of(21, 2, 0, vw), index_of(21, 2, vw - 1, vw), index_of(21, 2, 1, vw)]
    g = np.random.default_rng(3)
    hm, hmf = (torch.from_numpy(g.uniform(-0.5, 0.5, size=(1, 17, H * W)).astype(F32)).to(dtype).float().numpy() for _ in range(2))
    partner, sx = partner_np(), src_x_np(W, shift)
    for j, where in cases.items():
        assert len(set(where)) == len(where) and max(where) < H * W
        for turn, i in enumerate(sorted(where)):
            y, x = divmod(i, W)
            src = y * W + sx[x]
            made_by = ("direct", "flipped", "both")[(turn + j) % 3] if not (shift and x <= 1) else "direct"      # (columns 0 and 1 share one flipped source)
            hm[0, j, i], hmf[0, partner[j], src] = {"direct": (1.5, 0.0), "flipped": (0.0, 1.5), "both": (0.75, 0.75)}[made_by]
    hm, hmf = hm.reshape(1, 17, H, W), hmf.reshape(1, 17, H, W)
    center, scale, _ = geometry(1, seed=9)
    dev = [torch.from_numpy(a).cuda() for a in (hm, hmf)]
    dev = [one_in(t) for t in dev] if path == "elementwise" else [t.to(dtype) for t in dev]
    assert all(torch.equal(t.float().cpu(), torch.from_numpy(a)) for t, a in zip(dev, (hm, hmf)))
    want, pos, _, merged = heatmap_flip_decode_np(hm, hmf, center, scale, shift=shift, parts=True)
    for j, where in cases.items():
        assert merged[0, j].max() == 0.75 and np.flatnonzero(merged[0, j].reshape(-1) == 0.75).tolist() == sorted(where), j
        assert pos[0, j, 1] * W + pos[0, j, 0] == min(where), (j, where)
    got = K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1], shift=shift)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (got.cpu() - torch.from_numpy(want)).abs().amax(dim=-1)


def test_nans_score_nan_and_leave_their_neighbours_alone():
    import kasportsformer_amd as K
    hm, hmf = pair_of_maps(2, 33, 31, seed=11)
    hm[0, 4, 20, 17] = np.nan                                   # a NaN in the direct operand only
    hmf[0, 5, 3, 30] = np.nan                                   # ... in the flipped operand only: it reaches merged map 6 (the partner of 5)
    hm[1, 1, 9, 8], hmf[1, 2, 9, 31 - 8] = np.inf, -np.inf      # +inf against -inf: a NaN like any other (src_x(8) = 31 - 8 with shift)
    hm[1, 3, 9, 8] = np.inf                                     # +inf alone: the score is inf, no NaN
    hm[1, 16, 32, 30] = np.nan                                  # the last value of the last map
    center, scale, _ = geometry(2, seed=12)
    want = heatmap_flip_decode_np(hm, hmf, center, scale)
    nan_scores = np.isnan(want[..., 2])
    assert sorted(map(tuple, np.argwhere(nan_scores))) == [(0, 4), (0, 6), (1, 1), (1, 16)] and want[1, 3, 2] == np.inf
    dev = torch.from_numpy(hm).cuda(), torch.from_numpy(hmf).cuda()
    got = K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1], merged=True)
    assert same(got.keypoints, want) and same(got.merged, merge_np(hm, hmf))
    clean = [np.where(np.isfinite(a), a, F32(0)) for a in (hm, hmf)]
    ordinary = torch.from_numpy(np.isfinite(want).all(axis=-1))
    got_clean = K.heatmaps_to_keypoints(clean[0], center, scale, flipped=clean[1])
    assert int(ordinary.sum()) == 34 - 5 and torch.equal(got.keypoints.cpu()[ordinary], got_clean.cpu()[ordinary])
    wide, widef = pair_of_maps(1, 64, 48, seed=13)              # the vector path: NaNs in the last slot of a lane's last load, in lane 0's first, in the flipped operand
    wide[0, 0].reshape(-1)[index_of(63, 11, 3, 4)] = np.nan
    wide[0, 1].reshape(-1)[[index_of(0, 0, 0, 4), index_of(5, 0, 2, 4)]] = np.nan
    widef[0, 3, 63, 0] = widef[0, 3, 0, 47] = np.nan            # the dropped column (nothing, with shift) and the edge column (merged columns 0 and 1 of map 4)
    for shift in (True, False):
        want = heatmap_flip_decode_np(wide, widef, center[:1], scale[:1], shift=shift)
        assert np.isnan(want[0, 4, 2]) and np.isnan(want[0, [0, 1], 2]).all()
        assert same(K.heatmaps_to_keypoints(torch.from_numpy(wide).cuda(), center[:1], scale[:1], flipped=torch.from_numpy(widef).cuda(), shift=shift), want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(64, 48), (7, 5)])
def test_sixteen_bit_heatmaps_decode_as_their_fp32_upcasts(H, W, dtype):
    """... which is not what half arithmetic on the tensors gives: the sum of two 16-bit values is kept in fp32."""
    import kasportsformer_amd as K
    n = 3
    center, scale, boxes = geometry(n, seed=21)
    if dtype == torch.float16 and (H, W) == (64, 48):
        fx = golden()
        a16, b16 = torch.from_numpy(fx["b_hm"][-n:]).cuda(), torch.from_numpy(fx["b_hmf"][-n:]).cuda()
    else:
        a16, b16 = (torch.from_numpy(a).cuda().to(dtype) for a in pair_of_maps(n, H, W, seed=22))
    keep = a16.clone(), b16.clone()
    for kw in (dict(center=center, scale=scale), dict(boxes=boxes, aspect=0.75, refine=False, shift=False)):
        got = K.heatmaps_to_keypoints(a16, flipped=b16, merged=True, **kw)
        up = K.heatmaps_to_keypoints(a16.float(), flipped=b16.float(), merged=True, **kw)
        assert torch.equal(got.keypoints, up.keypoints) and torch.equal(got.merged, up.merged)
        assert torch.equal(got.keypoints.cpu(), torch.from_numpy(heatmap_flip_decode_np(a16.cpu(), b16.cpu(), **kw)))
    if (H, W) == (7, 5):
        index = [torch.from_numpy(t).cuda() for t in (partner_np(), src_x_np(W, True))]
        half = ((a16 + b16[:, index[0]][..., index[1]]) * 0.5).float()
        assert not torch.equal(half, K.heatmaps_to_keypoints(a16, center, scale, flipped=b16, merged=True).merged), "half arithmetic rounds the sum"
    assert torch.equal(a16, keep[0]) and torch.equal(b16, keep[1])


def test_custom_pairs_and_no_pairs():
    import kasportsformer_amd as K
    hm, hmf = pair_of_maps(3, 33, 31, seed=41)
    center, scale, _ = geometry(3, seed=42)
    dev = torch.from_numpy(hm).cuda(), torch.from_numpy(hmf).cuda()
    results = []
    for pairs in (None, COCO_PAIRS, [(5, 6)], [], [(0, 16), (3, 2)]):
        table = partner_np(COCO_PAIRS if pairs is None else pairs)
        got = K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1], pairs=pairs, merged=True)
        assert torch.equal(got.keypoints.cpu(), torch.from_numpy(heatmap_flip_decode_np(hm, hmf, center, scale, partner=table)))
        assert torch.equal(got.merged.cpu(), torch.from_numpy(merge_np(hm, hmf, partner=table)))
        results.append(got.keypoints)
    assert torch.equal(results[0], results[1]) and not torch.equal(results[1], results[2]) and not torch.equal(results[2], results[3])


def test_h36m_layout_is_coco_to_h36m_of_the_coco_result():
    import kasportsformer_amd as K
    fx = golden()
    hm, hmf = torch.from_numpy(fx["a_hm"]).cuda(), torch.from_numpy(fx["a_hmf"]).cuda()
    kw = dict(center=fx["a_center"], scale=fx["a_scale"], flipped=hmf)
    coco = K.heatmaps_to_keypoints(hm, **kw)
    h36m = K.heatmaps_to_keypoints(hm, layout="h36m", **kw)
    assert isinstance(coco, torch.Tensor) and torch.equal(h36m, K.coco_to_h36m(coco)) and not torch.equal(h36m, coco)
    both = K.heatmaps_to_keypoints(hm, layout="h36m", merged=True, **kw)
    assert torch.equal(both.keypoints, h36m) and torch.equal(both.merged.cpu(), torch.from_numpy(fx["a_merged"]))
    assert not torch.equal(coco, K.heatmaps_to_keypoints(hm, fx["a_center"], fx["a_scale"])), "the flip test changes the keypoints"


def test_merged_into_a_callers_tensor_writes_all_of_it_and_nothing_else():
    import kasportsformer_amd as K
    n, H, W = 3, 6, 8
    hm, hmf = pair_of_maps(n, H, W, seed=51)
    center, scale, _ = geometry(n, seed=52)
    dev = torch.from_numpy(hm).cuda(), torch.from_numpy(hmf).cuda()
    for dtype in (torch.float32, torch.float16):
        a, b = dev[0].to(dtype), dev[1].to(dtype)
        store = torch.full((n + 1, 17, H, W), -7.5, device="cuda")
        target = store[:n]
        got = K.heatmaps_to_keypoints(a, center, scale, flipped=b, merged=target)
        assert got.merged is target and got.merged.data_ptr() == store.data_ptr()
        assert torch.equal(target.cpu(), torch.from_numpy(merge_np(a.cpu(), b.cpu()))) and bool((store[n] == -7.5).all()), "the row after it is untouched"
        plain = K.heatmaps_to_keypoints(a, center, scale, flipped=b)
        fresh = K.heatmaps_to_keypoints(a, center, scale, flipped=b, merged=True)
        assert isinstance(plain, torch.Tensor) and torch.equal(plain, got.keypoints) and torch.equal(plain, fresh.keypoints)
        assert torch.equal(fresh.merged, target)
    odd = torch.full((n * 17 * H * W + 1,), -7.5, device="cuda")          # a target that is not 16-byte aligned: the element-wise path, the same values
    target = odd[1:].view(n, 17, H, W)
    got = K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1], merged=target)
    assert torch.equal(target.cpu(), torch.from_numpy(merge_np(hm, hmf))) and odd[0] == -7.5
    assert torch.equal(got.keypoints, K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1]))
    with pytest.raises(ValueError):
        K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1], merged=store)                    # one person too many
    with pytest.raises(ValueError):
        K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1], merged=store[:n].transpose(-1, -2))
    for own in dev:
        with pytest.raises(ValueError):
            K.heatmaps_to_keypoints(dev[0], center, scale, flipped=dev[1], merged=own)                  # an input as the target
    assert torch.equal(dev[0].cpu(), torch.from_numpy(hm)) and torch.equal(dev[1].cpu(), torch.from_numpy(hmf))


def test_the_same_bits_again_and_for_a_person_alone_or_in_a_batch():
    import kasportsformer_amd as K
    fx = golden()
    hm, hmf = torch.from_numpy(fx["b_hm"]).cuda(), torch.from_numpy(fx["b_hmf"]).cuda()
    center, scale = torch.from_numpy(fx["b_center"]).cuda(), torch.from_numpy(fx["b_scale"]).cuda()
    first = K.heatmaps_to_keypoints(hm, center, scale, flipped=hmf)
    assert torch.equal(first, K.heatmaps_to_keypoints(hm, center, scale, flipped=hmf))
    for p in range(hm.shape[0]):
        assert torch.equal(K.heatmaps_to_keypoints(hm[p], center[p], scale[p], flipped=hmf[p]), first[p])
    host = K.heatmaps_to_keypoints(fx["b_hm"], fx["b_center"], fx["b_scale"], flipped=fx["b_hmf"])        # host input is uploaded
    strided = K.heatmaps_to_keypoints(hm[::2], center[::2], scale[::2], flipped=hmf[::2])                 # strided views are packed
    assert torch.equal(host, first) and torch.equal(strided, first[::2])


def test_entry_point_refuses_device_pointers_too():
    from kasportsformer_amd import _lib
    import ctypes as C
    lib = _lib.load()
    hm, hmf, geom = torch.ones(17 * 15, device="cuda"), torch.ones(17 * 15, device="cuda"), torch.ones(4, device="cuda")
    out, mrg = torch.full((51,), 7.0, device="cuda"), torch.full((17 * 15,), 7.0, device="cuda")
    f = lib.kasf_heatmap_flip_keypoints
    bad = np.arange(17, dtype=np.int32)
    bad[[1, 2, 3]] = 2, 3, 1
    far = np.arange(17, dtype=np.int32)
    far[16] = 17
    table = lambda t: C.c_void_p(t.ctypes.data)
    # (hm, hm_flipped, dtype, n, H, W, partner, shift, geom, geom_kind, aspect, refine, out_layout, out, coco_scratch, merged_out, stream)
    for args in ((ptr(hm), None, 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, 0, ptr(out), None, ptr(mrg)),
                 (ptr(hm), ptr(hmf), 0, 1, 5, 3, table(bad), 1, ptr(geom), 0, 1.0, 1, 0, ptr(out), None, ptr(mrg)),
                 (ptr(hm), ptr(hmf), 0, 1, 5, 3, table(far), 1, ptr(geom), 0, 1.0, 1, 0, ptr(out), None, ptr(mrg)),
                 (ptr(hm), ptr(hmf), 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, 0, ptr(out), None, ptr(hm)),
                 (ptr(hm), ptr(hmf), 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, 0, ptr(out), None, ptr(hmf)),
                 (ptr(hm), ptr(hmf), 3, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, 0, ptr(out), None, ptr(mrg)),
                 (ptr(hm), ptr(hmf), 0, 1, 5, 3, None, 1, ptr(geom), 0, 1.0, 1, 1, ptr(out), None, ptr(mrg))):
        assert f(*args, stream()) == 2 and lib.kasf_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((mrg == 7).all()) and bool((hm == 1).all()) and bool((hmf == 1).all())


@pytest.mark.parametrize("layout,cd", [("h36m", "fp32"), ("coco", "bf16")])
def test_stream_push_heatmaps_is_push_of_the_decoded_keypoints(layout, cd):
    """A few ticks on 3 slots, with and without slots=: push_heatmaps(flipped=...) on one lifter, push of heatmaps_to_keypoints(flipped=...)'s result on a second."""
    import kasportsformer_amd as K
    m = make_pair(1, 27, cd)[1].eval()
    S, H, W = 3, 16, 12
    a, b = (K.StreamLifter(m, 1920, 1080, slots=S, layout=layout) for _ in range(2))
    g = np.random.default_rng(51)
    for tick, (ids, kw) in enumerate(((None, {}), ([2, 0], dict(shift=False)), (None, dict(pairs=[(5, 6)])), ([1], {}))):
        k = S if ids is None else len(ids)
        hm, hmf = (torch.from_numpy(x).cuda() for x in pair_of_maps(k, H, W, seed=60 + tick))
        center = (g.uniform(0.2, 0.8, size=(k, 2)) * np.array([1920, 1080])).astype(F32)
        scale = g.uniform(1, 3, size=(k, 2)).astype(F32)
        keep = hm.clone(), hmf.clone()
        got = a.push_heatmaps(hm, center, scale, slots=ids, flipped=hmf, **kw)
        kp = K.heatmaps_to_keypoints(hm, center, scale, layout=layout, flipped=hmf, **kw)
        assert not torch.equal(kp, K.heatmaps_to_keypoints(hm, center, scale, layout=layout))
        want = b.push(kp, slots=ids)
        assert tuple(got.shape) == (k, 17, 3) and same(got, want), tick
        assert torch.equal(hm, keep[0]) and torch.equal(hmf, keep[1])
        assert np.array_equal(a.counts, b.counts)
    assert torch.equal(a._ring, b._ring)
    with pytest.raises(ValueError):
        a.push_heatmaps(hm, center, scale, slots=[1], flipped=hmf[:, :, :8])
    with pytest.raises(ValueError):
        a.push_heatmaps(hm, center, scale, slots=[1], pairs=[(5, 6)])
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
        hm, hmf = (torch.from_numpy(x).cuda() for x in pair_of_maps(n, 16, 12, seed=80 + tick))
        kw = (dict(), dict(shift=False), dict(pairs=[]))[tick]
        if tick == 1:
            got = pushed.push_heatmaps(hm.view(B, R, 17, 16, 12), center.view(B, R, 2), scale.view(B, R, 2), t, flipped=hmf.view(B, R, 17, 16, 12), **kw)
        else:
            got = pushed.push_heatmaps(hm, center, scale, t, flipped=hmf, **kw)
        want = decoded.push(K.heatmaps_to_keypoints(hm, center, scale, layout="h36m", flipped=hmf, **kw), t)
        assert all(torch.equal(u, v) for u, v in zip(got, want)), tick
        assert want.valid.any() and want.poses.abs().sum() > 0
    with pytest.raises(ValueError):
        pushed.push_heatmaps(hm, center, scale, t, flipped=hmf.half())
