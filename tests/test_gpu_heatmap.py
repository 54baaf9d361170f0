"""The heatmap decode on the device (kasf_heatmap_keypoints, K.heatmaps_to_keypoints, StreamLifter.push_heatmaps) against the numpy restatement of
tests/test_heatmap_cpu.py, which that file ties to the reference's own outputs.  Device and restatement perform the same IEEE operations, so every comparison
is exact (torch.equal; where a NaN is expected, equal NaN positions and equal values elsewhere).  Nothing here provokes a fault: refusals are tested through
the error code.

The kernel's mapping (k_heatmap_keypoints in csrc/k_heatmap.hip, which the flip-tested kernel shares its helpers with), which the tie tests place their maxima by: one wavefront per map; a map is read as vectors of VW values (16 bytes:
VW = 4 for fp32, 8 for fp16 / bf16; VW = 1 on the element-wise path, taken when the array does not start on a 16-byte boundary or a map is not a multiple of 16
bytes); vector v is read by lane v % 64 in that lane's pass v // 64, and value k of it is map index v * VW + k."""
import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.test_heatmap_cpu import F32, GROUPS, fixture, heatmap_decode_np

pytestmark = pytest.mark.gpu


def index_of(lane, lane_pass, slot, vw):
    """Map index of value `slot` of the vector that `lane` reads in its pass number `lane_pass`."""
    return ((lane_pass * 64 + lane) * vw) + slot


def same(got: torch.Tensor, want) -> bool:
    """Equal, a NaN equal to a NaN."""
    want = torch.as_tensor(want).to(got.device)
    return got.shape == want.shape and torch.equal(got.isnan(), want.isnan()) and torch.equal(torch.where(got.isnan(), 0.0, got), torch.where(want.isnan(), 0.0, want))


def geometry(n, seed=0, frame=(1920.0, 1080.0)):
    g = np.random.default_rng(seed)
    center = (g.uniform(0, 1, size=(n, 2)) * np.array(frame)).astype(F32)
    scale = g.uniform(0.3, 4.0, size=(n, 2)).astype(F32)
    x1, y1 = g.uniform(0, frame[0] / 2, n), g.uniform(0, frame[1] / 2, n)
    boxes = np.stack((x1, y1, x1 + g.uniform(20, 400, n), y1 + g.uniform(40, 500, n)), axis=-1).astype(F32)
    return center, scale, boxes


def random_maps(n, H, W, seed=0):
    return np.random.default_rng(seed).normal(size=(n, 17, H, W)).astype(F32)


_FIXTURE = {}


def golden():
    if not _FIXTURE:
        fx = fixture()
        _FIXTURE.update({k: fx[k] for k in fx.files})
    return _FIXTURE


@pytest.mark.parametrize("kind", ["center_scale", "box"])
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_fixture_decodes_to_the_restatement(group, refine, kind):
    """Both map sizes (96 x 72, 64 x 48), refine on and off, both geometry kinds, COCO out: blobs, and the hand-made person -- two and three equal maxima, an
    all-zero and an all-negative map, peaks at px / py in {0, 1, size - 2, size - 1}, equal neighbours on one axis (tests/golden/make_heatmap_golden.py)."""
    import kasportsformer_amd as K
    fx = golden()
    hm = torch.from_numpy(fx[group + "_hm"].astype(F32)).cuda()
    keep = hm.clone()
    if kind == "box":
        kw = dict(boxes=fx[group + "_boxes"], aspect=float(fx[group + "_aspect"]))
    else:
        kw = dict(center=fx[group + "_center"], scale=fx[group + "_scale"])
    got = K.heatmaps_to_keypoints(hm, refine=refine, **kw)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (hm.shape[0], 17, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(heatmap_decode_np(fx[group + "_hm"], refine=refine, **kw)))
    assert torch.equal(hm, keep), "the heatmaps are only read"


@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("H,W", [(5, 3), (7, 5), (4, 4), (6, 8), (33, 31), (64, 48), (96, 72)])
def test_map_shapes_and_map_count_tails(H, W, n):
    """Maps smaller than a wavefront and not a multiple of 4 values (5 x 3, 7 x 5: element-wise path), vector path with idle lanes (4 x 4, 6 x 8), an odd size
    over several passes (33 x 31), the two network sizes; n * 17 = 17, 51, 85 maps is never a multiple of the 4 maps of a workgroup."""
    import kasportsformer_amd as K
    hm = random_maps(n, H, W, seed=H * 100 + n)
    center, scale, boxes = geometry(n, seed=n)
    dev_hm, dev_c, dev_s = torch.from_numpy(hm).cuda(), torch.from_numpy(center).cuda(), torch.from_numpy(scale).cuda()
    for refine in (True, False):
        got = K.heatmaps_to_keypoints(dev_hm, dev_c, dev_s, refine=refine)
        assert torch.equal(got.cpu(), torch.from_numpy(heatmap_decode_np(hm, center, scale, refine=refine)))
    got = K.heatmaps_to_keypoints(dev_hm, boxes=torch.from_numpy(boxes).cuda(), aspect=1080 / 1920)
    assert torch.equal(got.cpu(), torch.from_numpy(heatmap_decode_np(hm, boxes=boxes, aspect=1080 / 1920)))
    assert torch.equal(dev_hm.cpu(), torch.from_numpy(hm)) and torch.equal(dev_c.cpu(), torch.from_numpy(center))


def test_no_persons_is_no_work():
    import kasportsformer_amd as K
    from kasportsformer_amd import _lib
    empty = K.heatmaps_to_keypoints(torch.zeros((0, 17, 5, 3), device="cuda"), torch.zeros((0, 2)), torch.zeros((0, 2)))
    assert tuple(empty.shape) == (0, 17, 3) and empty.is_cuda
    assert tuple(K.heatmaps_to_keypoints(np.zeros((2, 0, 17, 5, 3), F32), np.zeros((2, 0, 2), F32), np.zeros((2, 0, 2), F32), layout="h36m").shape) == (2, 0, 17, 3)
    out = torch.full((51,), 7.0, device="cuda")
    hm, geom = torch.zeros(17 * 15, device="cuda"), torch.ones(4, device="cuda")
    assert _lib.load().kasf_heatmap_keypoints(ptr(hm), 0, 0, 5, 3, ptr(geom), 0, 1.0, 1, 1, ptr(out), ptr(out), stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "n = 0 leaves the output alone"


@pytest.mark.parametrize("path", ["fp32", "fp16", "bf16", "elementwise"])
def test_equal_maxima_go_to_the_first_in_row_major_order(path):
    """Two and three equal maxima placed by the kernel's mapping (module docstring): in different lanes with the FIRST one in the higher lane and a later pass
    of its lane's competitor, in one lane in two passes, and in two slots of one vector load.  64 x 48 maps = 3,072 values: 12 passes of VW = 4, 6 of VW = 8,
    48 on the element-wise path."""
    import kasportsformer_amd as K
    H, W = 64, 48
    vw = {"fp32": 4, "fp16": 8, "bf16": 8, "elementwise": 1}[path]
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(path, torch.float32)
    last = 3072 // (64 * vw) - 1
    first = index_of(50, 1, 1, vw)                              # lane 50, pass 1
    cases = {
        0: [first, index_of(10, 3, max(vw - 2, 0), vw)],                                  # a lower lane holds the later one
        1: [first, index_of(10, 3, max(vw - 2, 0), vw), index_of(10, last, 0, vw)],       # three: two of them in lane 10
        2: [index_of(7, 2, 0, vw), index_of(7, last, vw - 1, vw)],                # one lane, two passes
        3: [index_of(63, 0, vw - 1, vw), index_of(0, 1, 0, vw)],                  # the last lane's value comes before lane 0's next pass
        4: [index_of(0, last, 0, vw), index_of(63, last, vw - 1, vw)],            # the very last vector of the map
        5: [index_of(31, 2, 0, vw), index_of(32, 2, 0, vw)],                      # neighbouring lanes, across the halves of the wave
    }
    if vw > 1:
        cases[6] = [index_of(20, 2, 1, vw), index_of(20, 2, 3, vw)]               # two slots of one 16-byte load
        cases[7] = [index_of(21, 2, 0, vw), index_of(21, 2, vw - 1, vw), index_of(21, 2, 1, vw)]
    hm = np.random.default_rng(3).uniform(-0.5, 0.5, size=(1, 17, H * W)).astype(F32)
    hm = hm.astype(np.float16).astype(F32) if path != "bf16" else torch.from_numpy(hm).bfloat16().float().numpy()
    for j, where in cases.items():
        assert len(set(where)) == len(where) and max(where) < H * W
        hm[0, j, where] = 0.75
    hm = hm.reshape(1, 17, H, W)
    center, scale, _ = geometry(1, seed=9)
    if path == "elementwise":
        store = torch.zeros(hm.size + 1, device="cuda")
        store[1:] = torch.from_numpy(hm).reshape(-1)
        dev = store[1:].view(1, 17, H, W)
        assert dev.data_ptr() % 16 == 4
    else:
        dev = torch.from_numpy(hm).cuda().to(dtype)
        assert dev.data_ptr() % 16 == 0 and torch.equal(dev.float().cpu(), torch.from_numpy(hm))
    want, pos, _ = heatmap_decode_np(hm, center, scale, parts=True)
    for j, where in cases.items():
        assert pos[0, j, 1] * W + pos[0, j, 0] == min(where), (j, where)
    got = K.heatmaps_to_keypoints(dev, center, scale)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (got.cpu() - torch.from_numpy(want)).abs().amax(dim=-1)


def test_a_nan_map_scores_nan_and_leaves_its_neighbours_alone():
    import kasportsformer_amd as K
    hm = random_maps(2, 33, 31, seed=11)
    hm[0, 4, 20, 17] = hm[0, 4, 3, 30] = np.nan                 # two NaNs in one map: the first one is the argmax, the score is NaN
    hm[1, 16, 32, 30] = np.nan                                  # the last value of the last map
    hm[1, 2] = 0
    hm[1, 2, 9, 8], hm[1, 2, 9, 7], hm[1, 2, 9, 9] = 1, -np.inf, -np.inf       # -inf - -inf: a NaN difference gives a NaN x, the score stays 1
    center, scale, _ = geometry(2, seed=12)
    want = heatmap_decode_np(hm, center, scale)
    assert np.isnan(want[0, 4, 2]) and np.isnan(want[1, 16, 2]) and np.isnan(want[1, 2, 0]) and want[1, 2, 2] == 1 and np.isnan(want).sum() == 3
    got = K.heatmaps_to_keypoints(torch.from_numpy(hm).cuda(), center, scale)
    assert same(got, want)
    clean = np.where(np.isnan(hm), F32(0), hm)
    ordinary = ~np.isnan(want).any(axis=-1)
    got_clean = K.heatmaps_to_keypoints(torch.from_numpy(clean).cuda(), center, scale)
    assert torch.equal(got.cpu()[torch.from_numpy(ordinary)], got_clean.cpu()[torch.from_numpy(ordinary)])
    wide = random_maps(1, 64, 48, seed=13)                      # the vector path: a NaN in the last slot of a lane's last load, and in lane 0's first
    wide[0, 0].reshape(-1)[index_of(63, 11, 3, 4)] = np.nan
    wide[0, 1].reshape(-1)[[index_of(0, 0, 0, 4), index_of(5, 0, 2, 4)]] = np.nan
    assert same(K.heatmaps_to_keypoints(torch.from_numpy(wide).cuda(), center[:1], scale[:1]), heatmap_decode_np(wide, center[:1], scale[:1]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(64, 48), (7, 5)])
def test_sixteen_bit_heatmaps_decode_as_their_fp32_upcast(H, W, dtype):
    import kasportsformer_amd as K
    n = 3
    center, scale, boxes = geometry(n, seed=21)
    if dtype == torch.float16 and (H, W) == (64, 48):
        fx = golden()
        hm16 = torch.from_numpy(fx["b_hm"][-n:]).cuda()         # blobs and the hand-made person, as stored
    else:
        hm16 = torch.from_numpy(random_maps(n, H, W, seed=22)).cuda().to(dtype)
    keep = hm16.clone()
    up = hm16.float()
    for kw in (dict(center=center, scale=scale), dict(boxes=boxes, aspect=0.75, refine=False)):
        got = K.heatmaps_to_keypoints(hm16, **kw)
        assert torch.equal(got, K.heatmaps_to_keypoints(up, **kw))
        assert torch.equal(got.cpu(), torch.from_numpy(heatmap_decode_np(up.cpu().numpy(), **kw)))
    assert torch.equal(hm16, keep)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_a_view_that_starts_one_element_in_takes_the_elementwise_path(dtype):
    import kasportsformer_amd as K
    n, H, W = 3, 64, 48
    hm = torch.from_numpy(random_maps(n, H, W, seed=31)).cuda().to(dtype)
    store = torch.zeros(hm.numel() + 1, device="cuda", dtype=dtype)
    store[1:] = hm.reshape(-1)
    view = store[1:].view(n, 17, H, W)
    assert hm.data_ptr() % 16 == 0 and view.data_ptr() % 16 == hm.element_size() and view.is_contiguous()
    center, scale, _ = geometry(n, seed=32)
    got = K.heatmaps_to_keypoints(view, center, scale)
    assert torch.equal(got, K.heatmaps_to_keypoints(hm, center, scale))
    assert torch.equal(got.cpu(), torch.from_numpy(heatmap_decode_np(hm.float().cpu().numpy(), center, scale)))
    assert store[0] == 0 and torch.equal(store[1:], hm.reshape(-1))


def test_h36m_layout_is_coco_to_h36m_of_the_coco_result():
    import kasportsformer_amd as K
    fx = golden()
    hm = torch.from_numpy(fx["a_hm"]).cuda()
    kw = dict(center=fx["a_center"], scale=fx["a_scale"])
    coco = K.heatmaps_to_keypoints(hm, **kw)
    h36m = K.heatmaps_to_keypoints(hm, layout="h36m", **kw)
    assert torch.equal(h36m, K.coco_to_h36m(coco)) and not torch.equal(h36m, coco)
    assert torch.equal(coco, K.heatmaps_to_keypoints(hm, layout="coco", **kw))


def test_host_input_leading_dimensions_and_strided_views():
    import kasportsformer_amd as K
    hm = random_maps(6, 7, 5, seed=41)
    center, scale, _ = geometry(6, seed=42)
    want = torch.from_numpy(heatmap_decode_np(hm, center, scale))
    assert torch.equal(K.heatmaps_to_keypoints(hm, center, scale).cpu(), want)                                  # numpy on the host
    assert torch.equal(K.heatmaps_to_keypoints(torch.from_numpy(hm), torch.from_numpy(center).cuda(), scale).cpu(), want)
    got = K.heatmaps_to_keypoints(hm.reshape(2, 3, 17, 7, 5), center.reshape(2, 3, 2), scale.reshape(2, 3, 2))
    assert tuple(got.shape) == (2, 3, 17, 3) and torch.equal(got.cpu().view(6, 17, 3), want)
    one = K.heatmaps_to_keypoints(hm[0], center[0], scale[0])
    assert tuple(one.shape) == (17, 3) and torch.equal(one.cpu(), want[0])
    dev = torch.from_numpy(hm).cuda()
    assert torch.equal(K.heatmaps_to_keypoints(dev[::2], center[::2], scale[::2]).cpu(), want[::2])             # a strided view is packed first
    with pytest.raises(RuntimeError):
        K.heatmaps_to_keypoints(dev, center, scale, device="cpu")


def test_entry_point_refuses_device_pointers_too():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    hm, geom, out = torch.ones(17 * 15, device="cuda"), torch.ones(4, device="cuda"), torch.full((51,), 7.0, device="cuda")
    f = lib.kasf_heatmap_keypoints
    for args in ((ptr(hm), 0, -1, 5, 3, ptr(geom), 0, 1.0, 1, 0, ptr(out), None),
                 (ptr(hm), 3, 1, 5, 3, ptr(geom), 0, 1.0, 1, 0, ptr(out), None),
                 (ptr(hm), 0, 1, 5, 3, ptr(geom), 1, 0.0, 1, 0, ptr(out), None),
                 (ptr(hm), 0, 1, 5, 3, ptr(geom), 0, 1.0, 1, 1, ptr(out), None),
                 (ptr(hm), 0, 1, 4097, 4096, ptr(geom), 0, 1.0, 1, 0, ptr(out), None)):
        assert f(*args, stream()) == 2 and lib.kasf_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all())


@pytest.mark.parametrize("layout,cd", [("h36m", "fp32"), ("coco", "bf16")])
def test_push_heatmaps_is_push_of_the_decoded_keypoints(layout, cd):
    """A few ticks on 3 slots, with and without slots=: push_heatmaps on one lifter, push of heatmaps_to_keypoints' result on a second one."""
    import kasportsformer_amd as K
    m = make_pair(2, 27, cd)[1].eval()
    S, H, W = 3, 33, 31
    a, b = (K.StreamLifter(m, 1920, 1080, slots=S, layout=layout) for _ in range(2))
    g = np.random.default_rng(51)
    for tick, ids in enumerate((None, None, [2, 0], None, [1])):
        k = S if ids is None else len(ids)
        hm = torch.from_numpy(random_maps(k, H, W, seed=60 + tick)).cuda()
        center = (g.uniform(0.2, 0.8, size=(k, 2)) * np.array([1920, 1080])).astype(F32)
        scale = g.uniform(1, 3, size=(k, 2)).astype(F32)
        keep = hm.clone()
        got = a.push_heatmaps(hm, center, scale, slots=ids)
        want = b.push(K.heatmaps_to_keypoints(hm, center, scale, layout=layout), slots=ids)
        assert tuple(got.shape) == (k, 17, 3) and same(got, want), tick
        assert same(hm, keep)
        assert np.array_equal(a.counts, b.counts)
    assert torch.equal(a._ring, b._ring)
    boxes = geometry(S, seed=52)[2]
    hm = torch.from_numpy(random_maps(S, H, W, seed=70)).cuda().half()
    got = a.push_heatmaps(hm, boxes=boxes, aspect=1080 / 1920, refine=False)
    assert same(got, b.push(K.heatmaps_to_keypoints(hm, boxes=boxes, aspect=1080 / 1920, refine=False, layout=layout)))
    with pytest.raises(ValueError):
        a.push_heatmaps(hm[:2], boxes=boxes[:2], aspect=0.5)    # two persons for three slots
    with pytest.raises(ValueError):
        a.push_heatmaps(hm, boxes=boxes)
    assert np.array_equal(a.counts, b.counts), "a refused call leaves the state as it was"
