"""The two matching rules of include/kasf.h (kasf_match_pair_costs, kasf_match_groups) as tests/match_ref.py restates them, without a GPU: the restatement's
port of csrc/assignment.h's augmenting-path walk against scipy's linear_sum_assignment by total cost; the rules' properties on a synthetic scene against the
known truth -- a ring of 5 cameras, 6 players, rows permuted per camera, one lens with distortion, a pixel of noise, a player absent from two cameras, another
seen by one camera only, an empty padded row --; and the degenerate cases.  The device and the host-compiled kernels are held to this restatement bit for bit
elsewhere; here the restatement itself is shown to do what the rule is for."""
import numpy as np
import pytest

from tests.match_ref import BIG, assign_np, groups_np, pair_costs_np, partition_of, project, ring, scene, truth_partition


@pytest.mark.parametrize("na,nb,kind", [(1, 1, "real"), (5, 5, "real"), (7, 3, "real"), (3, 7, "real"), (64, 64, "real"), (64, 17, "grid"), (17, 64, "grid"),
                                        (40, 40, "grid"), (64, 64, "big"), (20, 33, "big"), (33, 20, "big"), (64, 64, "grid")])
def test_the_walk_finds_the_least_total_cost(na, nb, kind):
    scipy_optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(na * 100 + nb)
    for _ in range(3):
        M = rng.uniform(0.0, 50.0, (na, nb)) if kind != "grid" else rng.integers(0, 6, (na, nb)) * 0.25          # a grid of quarter pixels: exact ties
        if kind == "big":
            M[rng.random((na, nb)) < 0.4] = BIG
        b_of_a, a_of_b = assign_np(M)
        pairs = [(a, b) for a, b in enumerate(b_of_a) if b >= 0]
        assert len(pairs) == min(na, nb) and len({b for _, b in pairs}) == len(pairs)
        assert all(a_of_b[b] == a for a, b in pairs) and (a_of_b >= 0).sum() == len(pairs)
        rows, cols = scipy_optimize.linear_sum_assignment(M)
        best, got = M[rows, cols].sum(), sum(M[a, b] for a, b in pairs)
        assert abs(got - best) <= 1e-9 * max(1.0, abs(best)), (got, best)
        again = assign_np(M.copy())
        assert np.array_equal(again[0], b_of_a) and np.array_equal(again[1], a_of_b)


@pytest.fixture(scope="module")
def stadium():
    K, cams, X, row = scene(frames=12, cameras=5, players=6, joints=17, pad=1, seed=0)
    cost, samples = pair_costs_np(K, cams)
    return K, cams, X, row, cost, samples, groups_np(cost, samples)


def test_the_scene_is_what_it_says(stadium):
    K, cams, _, row, _, _, _ = stadium
    assert K.shape == (5, 7, 12, 17, 3) and (cams[1, 4:9] != 0).all() and (cams[[0, 2, 3, 4], 4:9] == 0).all()
    assert (row[:, :4] >= 0).all() and row[:, 4].tolist().count(-1) == 2 and (row[:, 5] >= 0).sum() == 1 and row[2, 5] >= 0
    assert any(sorted(r[r >= 0]) != list(range((r >= 0).sum())) for r in row)                  # the rows are permuted
    assert all(((K[c, :, :, :, 2] == 0).all((1, 2))).sum() >= 1 for c in range(5))              # every camera has an empty row


def test_the_cost_is_symmetric_and_separates_true_from_false_pairs(stadium):
    _, _, _, row, cost, samples, _ = stadium
    for a in range(5):
        assert np.isinf(cost[a, a]).all() and (samples[a, a] == 0).all()
        for b in range(5):
            assert np.array_equal(cost[a, b].view(np.uint32), cost[b, a].T.view(np.uint32)) and np.array_equal(samples[a, b], samples[b, a].T)
    true = [cost[a, b, row[a, i], row[b, i]] for i in range(6) for a in range(5) for b in range(5) if a != b and row[a, i] >= 0 and row[b, i] >= 0]
    false = [cost[a, b, row[a, i], row[b, j]] for i in range(6) for j in range(6) if i != j for a in range(5) for b in range(5)
             if a != b and row[a, i] >= 0 and row[b, j] >= 0]
    assert len(true) == 4 * 20 + 6 and max(true) < 15.0 < min(false)                           # max_cost = 15 px lies between them
    assert max(true) < 3.0                                                                      # a pixel of noise in each view: a gap of a pixel or two


def test_the_grouping_equals_the_truth(stadium):
    _, _, _, row, _, samples, g = stadium
    assert partition_of(g["members"]) == truth_partition(row) and g["count"] == 6 and g["dropped"] == 0
    for c in range(5):
        for i in range(6):
            if row[c, i] >= 0:
                grp = g["group"][c, row[c, i]]
                assert grp >= 0 and g["members"][grp, c] == row[c, i]
    alone = g["group"][2, row[2, 5]]                                                           # the player only camera 2 sees: a group of its own
    assert g["views"][alone] == 1 and np.isnan(g["group_cost"][alone]) and (g["members"][alone] >= 0).sum() == 1
    used = {(c, int(r)) for c in range(5) for r in row[c] if r >= 0}
    for c in range(5):                                                                         # empty rows stay at -1
        for r in range(7):
            assert ((c, r) in used) == (g["group"][c, r] >= 0)
    assert sorted(g["views"][:6].tolist()) == [1, 3, 5, 5, 5, 5] and (g["views"][6:] == 0).all() and (g["members"][6:] == -1).all()
    multi = g["views"] > 1
    assert (g["group_cost"][multi] < 3.0).all() and np.isnan(g["group_cost"][~multi]).all()


def test_too_few_groups_drop_the_rest_and_a_tight_bound_splits_the_players(stadium):
    _, _, _, _, cost, samples, _ = stadium
    few = groups_np(cost, samples, max_groups=3)
    assert few["count"] == 3 and few["dropped"] > 0 and (few["group"] < 3).all()
    tight = groups_np(cost, samples, max_cost=0.01)
    assert tight["count"] > 6 and (tight["views"][:tight["count"]] == 1).all()


def two_cameras(points, second=None):
    """Two cameras 8 m apart that look along +z, and the exact keypoints of world `points` [N,J,3] in them -> (K [2,1,N,J,3], cams [2,21])."""
    eye = np.eye(3).reshape(-1)
    cams = np.stack([np.concatenate([[1000, 1000, 960, 540], np.zeros(5), eye, t]) for t in ([0, 0, 0], [-8.0, 0, 0] if second is None else second)]).astype(np.float32)
    N, J = points.shape[:2]
    uv = project(points.reshape(-1, 3), cams)
    K = np.concatenate([uv, np.full((2, N * J, 1), 0.9)], -1).astype(np.float32).reshape(2, 1, N, J, 3)
    return K, cams


def test_degenerate_samples_are_not_comparable():
    pts = np.random.default_rng(3).uniform([-2, -1, 8], [10, 1, 12], (4, 5, 3))
    K, cams = two_cameras(pts)
    cost, samples = pair_costs_np(K, cams, min_samples=1)
    assert samples[0, 1, 0, 0] == 20 and cost[0, 1, 0, 0] < 1e-2                                # exact keypoints: the rays meet
    _, samples = pair_costs_np(*two_cameras(pts, second=[0, 0, 0]), min_samples=1)              # coincident centres
    assert samples[0, 1, 0, 0] == 0
    K2 = K.copy()
    K2[1] = K2[0]                                                                              # the same pixel in two cameras with one orientation: parallel rays
    cost, samples = pair_costs_np(K2, cams, min_samples=1)
    assert samples[0, 1, 0, 0] == 0 and np.isinf(cost[0, 1, 0, 0])
    K3 = K.copy()
    K3[0, ..., 0], K3[1, ..., 0] = 960.0 - 200.0, 960.0 + 200.0                                # rays that spread apart: they meet behind both cameras
    _, samples = pair_costs_np(K3, cams, min_samples=1)
    assert samples[0, 1, 0, 0] == 0


def test_min_samples_not_reached_is_infinite_and_unusable_keypoints_do_not_count():
    pts = np.random.default_rng(4).uniform([-2, -1, 8], [10, 1, 12], (3, 4, 3))
    K, cams = two_cameras(pts)
    assert np.isfinite(pair_costs_np(K, cams, min_samples=12)[0][0, 1, 0, 0]) and np.isinf(pair_costs_np(K, cams, min_samples=13)[0][0, 1, 0, 0])
    assert np.isinf(pair_costs_np(K, cams)[0]).sum() == 2 and np.isfinite(pair_costs_np(K, cams)[0][0, 1, 0, 0])      # the default 2 J = 8; the diagonal
    K[0, 0, 0, 0, 2], K[1, 0, 1, 1, 0], K[1, 0, 2, 2, 2] = 0.1, np.nan, np.nan
    assert pair_costs_np(K, cams)[1][0, 1, 0, 0] == 9
    cams[1, 20] = np.inf
    assert pair_costs_np(K, cams)[1].sum() == 0


def test_the_cap_bounds_what_one_sample_costs_and_the_weights_are_the_scores():
    K, cams, _, row = scene(frames=4, cameras=2, players=2, joints=5, pad=0, seed=2)
    cost, _ = pair_costs_np(K, cams, cap=7.0)
    assert np.isfinite(cost[0, 1]).all() and cost[0, 1].max() <= 7.0 and cost[0, 1].min() < 3.0
    K[0, row[0, 0], 0, 0, :2] += 400.0                                                         # one keypoint far off, scored low
    K[0, row[0, 0], 0, 0, 2] = 0.31
    w = pair_costs_np(K, cams)[0][0, 1, row[0, 0], row[1, 0]]
    u = pair_costs_np(K, cams, weighted=False)[0][0, 1, row[0, 0], row[1, 0]]
    assert w < u
