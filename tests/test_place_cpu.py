"""Properties of the camera-space placement's rule (include/kasf.h, kasf_pose_place) shown on its numpy restatement alone (tests/place_ref.py): what the
kernel is held to bit for bit elsewhere is right in the first place.  Synthetic players only: skeletons with the bone lengths of a 1.7 m person and random
bone directions, 4 - 40 m in front of a pinhole camera of f = 1500 px.  The bounds are the issue's; the measured values stand beside them."""
import numpy as np

from tests.place_ref import BONES_170, PARENTS, bundle, place_np, project, same_bits, scene
from tests.refine_ref import refine_np, weights


def depth_error(r, T):
    return np.abs(r["root"][:, 2].astype(np.float64) - T[:, 2]) / T[:, 2]


def test_exact_keypoints_recover_the_translation():
    """Keypoints projected exactly from the fp32 poses and rounded to fp32: max |T - T_true| / depth <= 1e-4 (measured 2e-6: the bound leaves room for the
    fp32 rounding of the keypoints, a hundredth of a pixel at x = 1900)."""
    P, T, K, camera = scene(np.random.default_rng(1), 500)
    r = place_np(P, K, camera, iterations=4)
    assert (r["state"] == 0).all()
    err = np.abs(r["root"].astype(np.float64) - T).max(1) / T[:, 2]
    print("max |T - T_true| / depth", err.max(), "max residual px", r["residual"].max())
    assert err.max() <= 1e-4
    assert r["residual"].max() < 0.01 and same_bits(r["scale"], np.ones(500, np.float32))
    assert np.allclose(r["poses"], P.astype(np.float64) + T[:, None, :], rtol=0, atol=1e-4 * 40)


def test_poses_times_two_double_the_result_bit_for_bit():
    P, T, K, camera = scene(np.random.default_rng(2), 500)
    K[..., :2] += np.random.default_rng(3).normal(0, 1, (500, 17, 2)).astype(np.float32)
    a, b = place_np(P, K, camera), place_np(P * np.float32(2), K, camera)
    assert (a["state"] == 0).all() and (b["state"] == 0).all()
    assert same_bits(b["root"], a["root"] * np.float32(2)) and same_bits(b["poses"], a["poses"] * np.float32(2))
    assert same_bits(b["residual"], a["residual"])


def noisy(seed, n, outlier):
    rng = np.random.default_rng(seed)
    P, T, K, camera = scene(rng, n)
    K[..., :2] += rng.normal(0.0, 1.0, (n, 17, 2)).astype(np.float32)
    if outlier:                                                          # one joint moved by (0.4, -0.3) of the player's pixel height
        height = K[..., 1].max(1) - K[..., 1].min(1)
        j = rng.integers(0, 17, n)
        K[np.arange(n), j, 0] += np.float32(0.4) * height
        K[np.arange(n), j, 1] -= np.float32(0.3) * height
    return P, T, K, camera


def test_reweighting_recovers_from_an_outlier_joint():
    """Median relative depth error with iterations=4, delta=3 at most one fifth of that with iterations=0 (measured 0.9 % against 31 %)."""
    P, T, K, camera = noisy(4, 300, True)
    plain, robust = place_np(P, K, camera, iterations=0), place_np(P, K, camera, iterations=4, delta=3.0)
    ok = (plain["state"] == 0) & (robust["state"] == 0)
    assert ok.sum() >= 290
    e0, e4 = np.median(depth_error(plain, T)[ok]), np.median(depth_error(robust, T)[ok])
    print("median relative depth error: iterations 0", e0, "iterations 4", e4)
    assert e4 <= e0 / 5


def test_reweighting_costs_nothing_on_clean_frames():
    """The same noise without the outlier: the medians differ by less than a tenth (measured 0.76 % against 0.79 %)."""
    P, T, K, camera = noisy(4, 300, False)
    plain, robust = place_np(P, K, camera, iterations=0), place_np(P, K, camera, iterations=4, delta=3.0)
    assert (plain["state"] == 0).all() and (robust["state"] == 0).all()
    e0, e4 = np.median(depth_error(plain, T)), np.median(depth_error(robust, T))
    print("median relative depth error, clean: iterations 0", e0, "iterations 4", e4)
    assert abs(e4 - e0) < 0.1 * e0


def bone_sum(poses, lengths):
    on = lengths > 0
    d = np.linalg.norm(poses[:, 1:].astype(np.float64) - poses[:, list(PARENTS)].astype(np.float64), axis=-1)
    return d[:, on].sum(1)


def test_a_metric_table_gives_roots_in_metres():
    """Poses in an arbitrary unit per frame and a table in metres: the roots come out in metres, and the placed bones sum to the table's sum."""
    rng = np.random.default_rng(6)
    P, T, K, camera = scene(rng, 200)
    unit = rng.uniform(0.01, 500.0, (200, 1, 1)).astype(np.float32)
    table = BONES_170.copy()
    table[9] = 0.0                                                       # a skipped bone takes no part in either sum
    r = place_np((P * unit).astype(np.float32), K, camera, table)
    assert (r["state"] == 0).all()
    assert np.allclose(r["scale"] * unit[:, 0, 0], 1.0, rtol=1e-5)
    assert (np.abs(r["root"].astype(np.float64) - T).max(1) / T[:, 2]).max() <= 1e-4
    assert np.allclose(bone_sum(r["poses"], table), table.astype(np.float64).sum(), rtol=1e-5)
    # the other route: poses made metric first, then no table
    again = place_np(P, K, camera)
    assert np.allclose(again["root"], r["root"], rtol=0, atol=1e-3)


def test_every_state():
    P, T, K, camera = scene(np.random.default_rng(7), 8)
    table = BONES_170
    few, point, behind, nan = K.copy(), K.copy(), K.copy(), P.copy()
    few[:, 3:, 2] = 0.1                                                  # three joints left, min_joints 4
    point[:, :, :2] = point[:, :1, :2]                                   # all keypoints in one point
    behind[..., :2] = project(P.astype(np.float64) + (T * [1, 1, -1])[:, None, :], camera).astype(np.float32)
    nan[:, 5, 2] = np.nan
    for name, (p, k, lengths), want in (("few", (P, few, None), 1), ("point", (P, point, None), 2), ("behind", (P, behind, None), 2), ("nan", (nan, K, table), 3),
                                        ("no bone", (P, K, np.zeros(16, np.float32)), 3), ("placed", (P, K, table), 0)):
        r = place_np(p, k, camera, lengths)
        assert (r["state"] == want).all(), (name, r["state"])
        if want:
            assert np.isnan(r["poses"]).all() and np.isnan(r["root"]).all() and np.isnan(r["residual"]).all()
        else:
            assert np.isfinite(r["poses"]).all() and np.isfinite(r["root"]).all() and np.isfinite(r["residual"]).all()
    assert (place_np(P, few, camera, min_joints=3)["state"] == 0).all()
    # without a table a pose value that is not finite only takes its joint out of the fit: the frame is placed, that joint stays not finite
    r = place_np(nan, K, camera)
    assert (r["state"] == 0).all() and np.isnan(r["poses"][:, 5, 2]).all() and np.isfinite(np.delete(r["poses"], 5, 1)).all()
    # too few joints comes before an unusable scale
    assert (place_np(nan, few, camera, table)["state"] == 1).all()


def test_frames_that_are_not_placed_are_nan_and_the_refinement_fills_them():
    n = 120
    rng = np.random.default_rng(8)
    P, _, _, camera = scene(rng, n)
    t = np.linspace(0.0, 1.0, n)
    T = np.stack([-3.0 + 6.0 * t, 0.5 * np.ones(n), 10.0 + 8.0 * t], 1)   # a player walking away on a straight line
    K = np.concatenate([project(P.astype(np.float64) + T[:, None, :], camera), np.full((n, 17, 1), 0.9)], -1).astype(np.float32)
    lost = (np.arange(n) % 17 == 5) | ((np.arange(n) >= 60) & (np.arange(n) < 66))
    K[lost, :, 2] = 0.0
    r = place_np(P, K, camera)
    assert np.array_equal(r["state"] != 0, lost) and np.isnan(r["root"][lost]).all() and np.isnan(r["poses"][lost]).all()
    w, radius = weights(2.0)
    root, st = refine_np(r["root"].reshape(n, 1, 3), np.array([0, n], np.int64), False, 0.3, 15, w, radius)
    assert np.array_equal(st[:, 0] == 1, lost) and np.isfinite(root).all()
    assert np.abs(root[:, 0].astype(np.float64) - T).max() < 1e-3         # the track is a line: interpolation and a symmetric window return it


def test_the_bundle_holds_every_state():
    for table in (False, True):
        P, K, camera, lengths = bundle(300, seed=1, table=table)
        st = place_np(P, K, camera, lengths)["state"]
        assert set(np.unique(st).tolist()) == ({0, 1, 2, 3} if table else {0, 1, 2})
        assert (st == 0).sum() > 150
