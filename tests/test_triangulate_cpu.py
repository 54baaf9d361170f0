"""The triangulation rule of include/kasf.h (kasf_keypoints_triangulate) as tests/triangulate_ref.py restates it, on synthetic players against the known truth:
what the rule promises, before any kernel is held to it.  Figures measured with this file are recorded in the docstrings; each test prints its own.

Permuting the views changes the order of the nine sums and so may change the last bits of a result: the rule fixes the order (views ascending) and no test here
asks for equality under a permutation."""
import numpy as np
import pytest

from tests.triangulate_ref import (LENS, bundle, holds_every_case, players, project, ring, same_bits, triangulate_np, triangulate_point, undistort_np)


def exact_keypoints(X, cams, score=0.9):
    uv = project(X, cams)
    return np.concatenate([uv, np.full(uv.shape[:-1] + (1,), score)], -1).astype(np.float32)


@pytest.mark.parametrize("views", [2, 3, 7, 16])
def test_exact_keypoints_give_the_point_back_to_fp32_rounding(views):
    """Keypoints projected in fp64 and rounded to fp32 carry 2^-24 of a 2,000 px coordinate, 6e-5 px: at 12 m and f = 1500 px that is half a micrometre
    per view, and the fp32 store of a coordinate of up to 5 m adds 2.4e-7 m.  Measured: 1.05e-6 m at 2 views, 5.5e-7 at 3, 4.1e-7 at 7, 3.4e-7 m at 16; the bar is 5e-6 m."""
    rng = np.random.default_rng(views)
    cams = ring(views, rng)
    X = players(rng, 30)
    r = triangulate_np(exact_keypoints(X, cams), cams, 17)
    err = np.abs(r["points"].astype(np.float64) - X).max()
    print(f"views {views}: max error {err:.3g} m, max residual {r['residual'].max():.3g} px")
    assert (r["state"] == 0).all() and (r["used"] == views).all()
    assert err < 5e-6 and r["residual"].max() < 1e-3


def test_undistort_inverts_the_forward_distortion():
    """k1 = -0.12, k2 = 0.05 (and the small p1, p2, k3 of tests/triangulate_ref.LENS), |x|, |y| <= 0.6, f = 1500 px: the fixed-point iteration contracts by
    about 0.13 per round at the corner.  Measured: 53 px at 0 rounds, 1.6e-2 px at 3, 1.8e-4 px at 5 and 1.25e-4 px at 20, where only the two fp32 roundings
    of a pixel coordinate below 2048 are left (6.1e-5 px each, the input's amplified by the inverse's slope of up to 1.2).  The bars: 3e-2 px at 3 rounds (a
    prototype's 2.2e-2 px), 4e-4 px at 5 (its 1.3e-4 px plus the roundings' 1.4e-4 px, with a margin) and 2.5e-4 px at 20."""
    rng = np.random.default_rng(5)
    f, cx, cy = 1500.0, 960.0, 540.0
    xy = rng.uniform(-0.6, 0.6, (4000, 2))
    cam = np.concatenate([[f, f, cx, cy], LENS, np.eye(3).reshape(-1), np.zeros(3)]).astype(np.float32)
    X = np.concatenate([xy, np.ones((4000, 1))], 1)
    K = exact_keypoints(X, cam[None])[0]
    ideal = np.stack([f * xy[:, 0] + cx, f * xy[:, 1] + cy], 1)
    err = {n: np.abs(undistort_np(K, cam[:9], 1, n)[:, :2].astype(np.float64) - ideal).max() for n in (0, 3, 5, 20)}
    print("undistort error in px by rounds:", {n: float(f"{e:.3g}") for n, e in err.items()})
    assert err[0] > 10.0                                                 # the lens is wrong by tens of pixels at the frame's edge
    assert err[3] < 3e-2 and err[5] < 4e-4 and err[20] < 2.5e-4
    assert same_bits(undistort_np(K, cam[:9], 1, 5)[:, 2], K[:, 2])


def test_undistort_then_pinhole_equals_the_lens_model_to_a_pixel_rounding():
    """Undistorting first and triangulating with zero coefficients differs from triangulating with the lens only by the fp32 rounding of the undistorted pixels."""
    K, cams, X = bundle(15, 7, seed=3, distortion=LENS)
    with_lens = triangulate_np(K, cams, 17)
    assert holds_every_case(with_lens, 7)
    flat = cams.copy()
    flat[:, 4:9] = 0.0
    Ku = np.stack([undistort_np(K[c], cams[c, :9], 17, 5) for c in range(7)])
    pinhole = triangulate_np(Ku, flat, 17, undistort_iterations=0)
    ok = (with_lens["state"] == 0) & (pinhole["state"] == 0)
    d = np.abs(with_lens["points"][ok].astype(np.float64) - pinhole["points"][ok]).max()
    print(f"lens model against undistort-then-pinhole: {d:.3g} m")
    assert np.array_equal(with_lens["used"], pinhole["used"]) and ok.sum() > 100 and d < 1e-5


def outlier_scene(views, seed, frames=40):
    """1 px of noise everywhere and, per point, one view displaced by 100 px -> (K, cams, X, which view)."""
    rng = np.random.default_rng(seed)
    cams = ring(views, rng)
    X = players(rng, frames)
    K = exact_keypoints(X, cams)
    K[..., :2] += rng.normal(0.0, 1.0, K[..., :2].shape).astype(np.float32)
    bad = rng.integers(0, views, len(X))
    a = rng.uniform(0.0, 2.0 * np.pi, len(X))
    K[bad, np.arange(len(X)), 0] += (100.0 * np.cos(a)).astype(np.float32)
    K[bad, np.arange(len(X)), 1] += (100.0 * np.sin(a)).astype(np.float32)
    return K, cams, X, bad


def test_reweighting_takes_a_displaced_view_out():
    """C = 7, 1 px of noise, one view per point displaced by 100 px.  Measured: median error 5.69 mm at iterations = 4 against 165 mm at iterations = 0, a
    ratio of 0.0345 (a prototype of the rule: 5.7 mm against 193 mm); the bar is a tenth.  The displaced view's own residual stays near 100 px."""
    K, cams, X, bad = outlier_scene(7, 11)
    med = {}
    for it in (0, 4):
        r = triangulate_np(K, cams, 17, iterations=it)
        assert (r["state"] == 0).all()
        med[it] = np.median(np.linalg.norm(r["points"].astype(np.float64) - X, axis=1))
    print(f"median error: {1e3 * med[4]:.3g} mm at iterations=4, {1e3 * med[0]:.3g} mm at iterations=0, ratio {med[4] / med[0]:.3g}")
    assert med[4] < 0.1 * med[0]
    own = r["view_residual"][bad, np.arange(len(X))]
    assert np.median(own) > 80.0 and np.median(np.delete(r["view_residual"], 0, 0)) < 5.0


def test_two_views_cannot_tell_which_one_is_wrong():
    """With C = 2 a displaced keypoint moves the point and both views share the error: the re-weighting has no third opinion to side with and cannot identify
    the wrong view.  Only that the residual is large is asserted (measured: a median of 35.3 px for a 100 px displacement, against 1.2e-5 px for the same points' exact keypoints)."""
    K, cams, X, _ = outlier_scene(2, 12)
    r = triangulate_np(K, cams, 17)
    clean = K.copy()
    clean[..., :2] = project(X, cams).astype(np.float32)
    r0 = triangulate_np(clean, cams, 17)
    print(f"median residual with a displaced view {np.nanmedian(r['residual']):.3g} px, without {np.nanmedian(r0['residual']):.3g} px")
    assert np.nanmedian(r["residual"]) > 10.0 and np.nanmedian(r0["residual"]) < 0.01


@pytest.mark.parametrize("views,per_frame,lens", [(3, False, False), (7, True, True), (16, False, True), (2, True, False)])
def test_a_point_alone_equals_the_point_in_the_batch_and_the_scalar_loop(views, per_frame, lens):
    """The batch form masks where the scalar loop of the header skips: the two agree bit for bit, point by point, on every output and in every state."""
    K, cams, _ = bundle(15, views, seed=20 + views, per_frame=per_frame, distortion=LENS if lens else None)
    full = triangulate_np(K, cams, 17)
    if views >= 3:
        assert holds_every_case(full, views)
    for n in range(0, K.shape[1], 3):
        rows = cams[:, n // 17] if per_frame else cams
        one = triangulate_np(K[:, n:n + 1], rows[:, None, :] if per_frame else rows, 1)
        X, res, used, state, vr = triangulate_point(K[:, n], rows)
        for k in ("points", "residual", "used", "state"):
            assert same_bits(one[k], full[k][n:n + 1]), (n, k)
        assert same_bits(one["view_residual"], full["view_residual"][:, n:n + 1]), n
        assert same_bits(X, full["points"][n]) and same_bits(np.float32(res), full["residual"][n]) and same_bits(vr, full["view_residual"][:, n]), n
        assert (used, state) == (int(full["used"][n]), int(full["state"][n])), n


def test_parameters_reach_the_scalar_loop_and_the_batch_alike():
    K, cams, _ = bundle(15, 7, seed=30, distortion=LENS)
    q = dict(min_score=0.55, weighted=False, iterations=1, delta=1.5, min_views=4, undistort_iterations=2)
    full = triangulate_np(K, cams, 17, **q)
    assert not same_bits(full["points"], triangulate_np(K, cams, 17)["points"]) and set(np.unique(full["state"]).tolist()) >= {0, 1}
    for n in range(0, K.shape[1], 5):
        X, res, used, state, vr = triangulate_point(K[:, n], cams, **q)
        assert same_bits(X, full["points"][n]) and same_bits(vr, full["view_residual"][:, n]) and (used, state) == (int(full["used"][n]), int(full["state"][n])), n


def test_states_leave_nan_for_refine_tracks():
    K, cams, _ = bundle(30, 7, seed=31)
    r = triangulate_np(K, cams, 17)
    assert holds_every_case(r, 7)
    off = r["state"] != 0
    assert np.isnan(r["residual"][off]).all() and np.isnan(r["view_residual"][:, off]).all() and np.isfinite(r["residual"][~off]).all()
    assert set(r["points"][off].view(np.uint32).reshape(-1).tolist()) == {0x7fc00000}
