"""Matching players across cameras on the GPU (kasportsformer_amd.match_players / match_costs / match_groups / gather_matched, csrc/k_match.hip): the public
functions and the C entries on the device equal the fp64 numpy restatement of include/kasf.h's two rules (tests/match_ref.py) bit for bit on cost, samples,
group, members, views, group_cost, count and dropped -- at one camera pair of one row and one sample; at 3 cameras of 5 rows with an empty row and uneven
lifetimes, 17 joints and 255, 256 and 257 frames (the 256-frame tile); at 16 cameras of 64 rows, the register / LDS ceiling, where 64 groups do not suffice --,
the grouping alone on planted costs with exact ties and BIG entries, sentinels behind every output, inputs unchanged, the same bits on a second run, a pair's
cost with only its two cameras given, a non-default stream, a call with no frames, and the chain to world joints.  A differing bit is a finding to explain,
not a bar to loosen.

The chain's check: gather_matched hands triangulate_keypoints, per group, exactly the tracks that the truth's grouping would, cameras in the same order, so the
points of every multi-view player must have the BITS of the triangulation of the truth-ordered tracks; and on the scene without pixel noise every joint of
every multi-view player lies within 2e-3 m of where it was put, the bound tests/test_gpu_triangulate.py holds its synthetic track to."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import ptr, stream
from tests.match_ref import groups_np, pair_costs_np, partition_of, scene, truth_partition

pytestmark = pytest.mark.gpu
GROUP_OUT = ("group", "members", "views", "group_cost", "count", "dropped")
TILE_FRAMES = (255, 256, 257)


def raw(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(got, want, name):
    assert tuple(got.shape) == tuple(np.shape(want)) and got.is_cuda, (name, tuple(got.shape), np.shape(want))
    g, w = raw(got), raw(want)
    assert g.size == w.size, name
    diff = np.flatnonzero(g != w)
    assert diff.size == 0, (name, diff[:8] // 4)


def same_costs(got, want):
    same(got.cost, want[0], "cost")
    same(got.samples, want[1], "samples")
    assert got.cost.dtype == torch.float32 and got.samples.dtype == torch.int32


def same_groups(got, want):
    for k in GROUP_OUT:
        same(getattr(got, k), want[k], k)
        assert getattr(got, k).dtype == (torch.float32 if k == "group_cost" else torch.int32)


@pytest.fixture(scope="module")
def cases():
    """The inputs and the restatement's outputs of the tests here, made once: name -> (K, cameras, (cost, samples), groups)."""
    out = {}
    for frames in TILE_FRAMES:
        K, cams, _, _ = scene(frames=frames, cameras=3, players=4, joints=17, pad=1, seed=frames, lifetimes=True)
        costs = pair_costs_np(K, cams)
        out[frames] = (K, cams, costs, groups_np(*costs))
    K, cams, _, _ = scene(frames=2, cameras=16, players=62, joints=3, pad=2, seed=5)
    costs = pair_costs_np(K, cams)
    out["ceiling"] = (K, cams, costs, groups_np(*costs, max_cost=1.0, max_groups=64))     # a pixel of noise: most pairs are rejected at 1 px
    return out


def test_one_camera_pair_of_one_row_and_one_sample():
    import kasportsformer_amd as K_
    K, cams, _, _ = scene(frames=1, cameras=2, players=1, joints=1, pad=0, seed=1)
    want = pair_costs_np(K, cams, min_samples=1)
    assert want[1][0, 1, 0, 0] == 1 and np.isfinite(want[0][0, 1, 0, 0])
    m = K_.match_players(K, cams, min_samples=1)
    assert isinstance(m, K_.MatchResult)
    same_costs(m, want)
    same_groups(m, groups_np(*want))
    assert int(m.count) == 1 and m.members.cpu().tolist() == [[0, 0], [-1, -1]]
    same_costs(K_.match_costs(K, cams), pair_costs_np(K, cams))         # min_samples = 2 J is not reached: +inf with one sample


@pytest.mark.parametrize("frames", TILE_FRAMES)
def test_three_cameras_of_five_rows_around_the_tile(cases, frames):
    import kasportsformer_amd as K_
    K, cams, costs, groups = cases[frames]
    assert (costs[1].sum((1, 3)) == 0).any() and np.isfinite(costs[0]).sum() >= 12 and groups["count"] >= 4 and (groups["views"] == 3).any()
    Kd, cd = torch.from_numpy(K).cuda(), torch.from_numpy(cams).cuda()
    m = K_.match_players(Kd, cd)
    same_costs(m, costs)
    same_groups(m, groups)
    again = K_.match_players(Kd, cd)                                    # the same bits on a second run
    same_costs(again, costs)
    same_groups(again, groups)
    host = K_.match_players([K[c] for c in range(3)], cams)             # numpy inputs on the host, as a list of C arrays
    same_costs(host, costs)
    same_groups(host, groups)
    assert np.array_equal(raw(Kd), raw(K)) and np.array_equal(raw(cd), raw(cams))


def test_a_pair_with_only_its_two_cameras_has_the_bits_it_has_among_three(cases):
    import kasportsformer_amd as K_
    K, cams, costs, _ = cases[257]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        two = K_.match_costs(K[[a, b]], cams[[a, b]])
        same(two.cost[0, 1], costs[0][a, b], (a, b))
        same(two.cost[1, 0], costs[0][b, a], (b, a))
        same(two.samples[0, 1], costs[1][a, b], (a, b))


def test_sixteen_cameras_of_sixty_four_rows_fill_every_group(cases):
    import kasportsformer_amd as K_
    K, cams, costs, groups = cases["ceiling"]
    assert groups["count"] == 64 and groups["dropped"] > 0 and (groups["views"] > 1).any()
    m = K_.match_players(K, cams, max_cost=1.0, max_groups=64)
    same_costs(m, costs)
    same_groups(m, groups)


def test_lists_with_different_row_counts_and_other_parameters(cases):
    import kasportsformer_amd as K_
    K, cams, _, _ = cases[255]
    q = dict(min_score=0.6, weighted=False, cap=20.0, min_samples=5, undistort_iterations=2)
    short = [K[0], K[1, :3], K[2, :4]]
    padded = K.copy()
    padded[1, 3:], padded[2, 4:] = 0.0, 0.0
    want = pair_costs_np(padded, cams, **q)
    m = K_.match_players(short, cams, max_cost=8.0, max_groups=3, **q)
    same_costs(m, want)
    same_groups(m, groups_np(*want, max_cost=8.0, max_groups=3))
    g = K_.gather_matched(short, m)
    members = m.members.cpu().numpy()
    assert tuple(g.shape) == (3, 3) + K.shape[2:] and g.is_cuda
    for c in range(3):
        for k in range(3):
            assert np.array_equal(raw(g[c, k]), raw(padded[c, members[k, c]] if members[k, c] >= 0 else np.zeros_like(K[0, 0])))


def planted(views, P, seed):
    """Costs on a grid of quarter pixels, so that exact ties abound, pairs without samples (BIG for a group of such members) and +inf costs."""
    rng = np.random.default_rng(seed)
    cost = (rng.integers(0, 12, (views, views, P, P)) * 0.25).astype(np.float32)
    samples = rng.integers(1, 4, (views, views, P, P)).astype(np.int32) * 10
    samples[rng.random(samples.shape) < 0.3] = 0
    cost[rng.random(cost.shape) < 0.2] = np.inf
    for a in range(views):
        for b in range(a, views):
            cost[b, a], samples[b, a] = cost[a, b].T, samples[a, b].T
        cost[a, a], samples[a, a] = np.inf, 0
    samples[:, :, P - 1, :] = samples[:, :, :, P - 1] = 0               # the last row of every camera is empty
    return cost, samples


@pytest.mark.parametrize("views,P,G,max_cost", [(2, 1, 1, 15.0), (3, 5, 10, 2.0), (4, 9, 6, 1.5), (16, 8, 64, 1.0), (3, 64, 64, 2.0), (5, 33, 40, 0.5)])
def test_the_grouping_alone_on_planted_costs_with_ties_and_big_entries(views, P, G, max_cost):
    import kasportsformer_amd as K_
    cost, samples = planted(views, P, views * 100 + P)
    want = groups_np(cost, samples, max_cost, G)
    if P > 4:
        assert (want["group"][:, P - 1] == -1).all() and want["count"] > 1 and (want["views"] > 1).any()
    got = K_.match_groups(cost, samples, max_cost=max_cost, max_groups=G)
    assert isinstance(got, K_.MatchGroups)
    same_groups(got, want)
    same_groups(K_.match_groups(torch.from_numpy(cost).cuda(), torch.from_numpy(samples).cuda(), max_cost=max_cost, max_groups=G), want)


@pytest.mark.parametrize("offset", [0, 1])
def test_the_entries_write_nothing_else(cases, offset):
    """The C entries with sentinels around every output and the workspace, at 16-byte aligned pointers and at pointers 4 bytes past them."""
    from kasportsformer_amd import _lib
    K, cams, costs, groups = cases[257]
    views, P, N, J = K.shape[:4]
    lib = _lib.load()
    src = torch.zeros(K.size + 8, device="cuda")
    src[offset:offset + K.size] = torch.from_numpy(K.reshape(-1)).cuda()
    Kd, cd = src[offset:offset + K.size], torch.from_numpy(cams).cuda()
    n = views * views * P * P
    nbytes = int(lib.kasf_match_workspace_bytes(views, P, N))
    assert nbytes == 20 * 2 * 3 * P * P
    cost, samples = torch.full((n + 128 + offset,), 9.0, device="cuda"), torch.full((n + 128 + offset,), 77, dtype=torch.int32, device="cuda")
    work = torch.full((nbytes // 4 + 128,), 77, dtype=torch.int32, device="cuda")
    lo = 64 + offset
    q = _lib.KasfMatchParams(0.3, 1, 50.0, 2 * J, 5)
    _lib.check(lib.kasf_match_pair_costs(ptr(Kd), views, P, N, J, ptr(cd), C.byref(q), ptr(cost[lo:]), ptr(samples[lo:]), ptr(work[64:]), nbytes, stream()))
    assert (cost[:lo] == 9.0).all() and (cost[lo + n:] == 9.0).all() and (samples[:lo] == 77).all() and (samples[lo + n:] == 77).all()
    assert (work[:64] == 77).all() and (work[64 + nbytes // 4:] == 77).all()
    assert np.array_equal(raw(cost[lo:lo + n]), raw(costs[0])) and np.array_equal(raw(samples[lo:lo + n]), raw(costs[1]))
    G = 2 * P
    sizes = dict(group=views * P, members=G * views, views=G, group_cost=G, count=1, dropped=1)
    outs = {k: torch.full((s + 128 + offset,), 77, dtype=torch.float32 if k == "group_cost" else torch.int32, device="cuda") for k, s in sizes.items()}
    _lib.check(lib.kasf_match_groups(ptr(cost[lo:]), ptr(samples[lo:]), views, P, 15.0, G, *[ptr(outs[k][lo:]) for k in GROUP_OUT], stream()))
    for k, s in sizes.items():
        assert (outs[k][:lo] == 77).all() and (outs[k][lo + s:] == 77).all(), k
        assert np.array_equal(raw(outs[k][lo:lo + s]), raw(groups[k])), k
    assert np.array_equal(raw(cost[lo:lo + n]), raw(costs[0])) and np.array_equal(raw(samples[lo:lo + n]), raw(costs[1]))       # the grouping only reads them
    assert np.array_equal(raw(Kd), raw(K)) and np.array_equal(raw(cd), raw(cams))


def test_a_non_default_stream_and_a_call_without_frames(cases):
    import kasportsformer_amd as K_
    K, cams, costs, groups = cases[256]
    Kd, cd = torch.from_numpy(K).cuda(), torch.from_numpy(cams).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m = K_.match_players(Kd, cd)
    side.synchronize()
    same_costs(m, costs)
    same_groups(m, groups)
    none = K_.match_players(K[:, :, :0], cams)                          # N = 0: no pair launch; every row is empty
    assert tuple(none.cost.shape) == (3, 3, 5, 5) and torch.isinf(none.cost).all() and (none.samples == 0).all()
    assert int(none.count) == 0 and int(none.dropped) == 0 and (none.group == -1).all() and (none.members == -1).all() and (none.views == 0).all()
    from kasportsformer_amd import _lib
    q = _lib.KasfMatchParams(0.3, 1, 50.0, 34, 5)
    assert _lib.load().kasf_match_pair_costs(None, 3, 5, 0, 17, None, C.byref(q), None, None, None, 0, None) == 0


def test_matched_gathered_and_triangulated_players_stand_where_they_stood():
    import kasportsformer_amd as K_
    for noise, seed in ((1.0, 0), (0.0, 0)):
        K, cams, X, row = scene(frames=12, cameras=5, players=6, joints=17, pad=1, seed=seed, noise=noise)
        m = K_.match_players(K, cams)
        members = m.members.cpu().numpy()
        assert partition_of(members) == truth_partition(row) and int(m.dropped) == 0
        points = K_.triangulate_keypoints(K_.gather_matched(K, m), cams).points
        assert tuple(points.shape) == (members.shape[0], 12, 17, 3)
        found = 0
        for i in range(6):
            seen = [c for c in range(5) if row[c, i] >= 0]
            if len(seen) < 2:
                continue
            g = int(m.group[seen[0], row[seen[0], i]])
            assert members[g].tolist() == row[:, i].tolist()
            truth = np.stack([K[c, row[c, i]] if row[c, i] >= 0 else np.zeros_like(K[0, 0]) for c in range(5)])
            assert np.array_equal(raw(points[g]), raw(K_.triangulate_keypoints(truth, cams).points))
            if noise == 0.0:
                assert np.abs(points[g].cpu().numpy().astype(np.float64) - X[i]).max() < 2e-3
            found += 1
        assert found == 5
