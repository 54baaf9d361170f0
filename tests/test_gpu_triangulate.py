"""The multi-camera triangulation and the undistortion on the GPU (kasportsformer_amd.triangulate_keypoints / undistort_keypoints, csrc/k_triangulate.hip): the
public functions and the C entries on the device equal the fp64 numpy restatement of include/kasf.h's rule (tests/triangulate_ref.py) bit for bit on points,
residual, used, state and view_residual -- at 1, 15, 16, 31 and 241 frames of 17 joints with 2, 7 and 16 cameras, at 257 points of one joint, with static and
per-frame cameras, with a lens --, the same bits on a second run, host and device inputs, a frame alone against the frame inside the batch, inputs unchanged,
sentinels behind the outputs intact at aligned and 4-byte-offset pointers, every state seen, and the NaN points filled by refine_tracks.  A differing bit is a
finding to explain, not a bar to loosen."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import ptr, stream
from tests.triangulate_ref import LENS, bundle, holds_every_case, triangulate_np, undistort_np

pytestmark = pytest.mark.gpu
FIELDS = ("points", "residual", "used", "state", "view_residual")
BYTES = ("used", "state")
CAN = 9.0
SHAPES = [(frames, views) for frames in (1, 15, 16, 31, 241) for views in (2, 7, 16)]


def raw(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def same(result, want, lead=None, fields=FIELDS):
    for name in fields:
        got, ref = getattr(result, name), want[name]
        if lead is not None:
            ref = ref.reshape(((ref.shape[0],) if name == "view_residual" else ()) + lead + ((3,) if name == "points" else ()))
        assert tuple(got.shape) == ref.shape and got.is_cuda and got.dtype == (torch.uint8 if name in BYTES else torch.float32), (name, tuple(got.shape), ref.shape)
        diff = np.argwhere(raw(got).reshape(-1) != raw(ref).reshape(-1))
        assert diff.size == 0, (name, diff[:8])


@pytest.fixture(scope="module")
def cases():
    """The inputs and the restatement's outputs of the tests here, made once: (frames, views) -> (K, cameras, want); frames of 17 joints, per-frame cameras at an
    odd frame count, a lens everywhere.  Key "points": 257 points of one joint."""
    out = {}
    for frames, views in SHAPES:
        K, cams, _ = bundle(frames, views, seed=frames + views, per_frame=frames % 2 == 1, distortion=LENS)
        out[frames, views] = (K, cams, triangulate_np(K, cams, 17))
    K, cams, _ = bundle(257, 3, seed=7, per_frame=True, distortion=LENS, joints=1)
    out["points"] = (K, cams, triangulate_np(K, cams, 1))
    return out


@pytest.mark.parametrize("frames,views", SHAPES)
def test_triangulate_keypoints_equals_the_restatement_bit_for_bit(cases, frames, views):
    import kasportsformer_amd as K_
    K, cams, want = cases[frames, views]
    if frames >= 15 and views >= 3:
        assert holds_every_case(want, views)
    lead = (frames, 17)
    K5 = K.reshape(views, frames, 17, 3)
    Kd, cd = torch.from_numpy(K5).cuda(), torch.from_numpy(cams).cuda()
    r = K_.triangulate_keypoints(Kd, cd, view_residual=True)
    assert isinstance(r, K_.TriangulateResult)
    same(r, want, lead)
    same(K_.triangulate_keypoints(Kd, cd, view_residual=True), want, lead)                        # the same bits on a second run
    host = K_.triangulate_keypoints([K5[c] for c in range(views)], cams)                          # numpy inputs on the host, as a list of C arrays
    assert host.view_residual is None
    same(host, want, lead, FIELDS[:4])
    assert np.array_equal(raw(Kd), raw(K5)) and np.array_equal(raw(cd), raw(cams))


def test_one_joint_per_frame_at_257_points(cases):
    import kasportsformer_amd as K_
    K, cams, want = cases["points"]
    assert holds_every_case(want, 3)
    same(K_.triangulate_keypoints(K.reshape(3, 257, 1, 3), cams, view_residual=True), want, (257, 1))


def test_other_parameters_and_leading_shapes(cases):
    import kasportsformer_amd as K_
    K, cams, _ = cases[16, 7]
    for q in (dict(iterations=0, undistort_iterations=0), dict(iterations=1, weighted=False, undistort_iterations=20),
              dict(iterations=8, delta=1.5, min_views=3, min_score=0.5)):
        same(K_.triangulate_keypoints(K.reshape(7, 16, 17, 3), cams, view_residual=True, **q), triangulate_np(K, cams, 17, **q), (16, 17))
    K, cams, want = cases[31, 7]                                                                  # per-frame cameras behind two leading dimensions
    six = {k: (v[:, :102] if k == "view_residual" else v[:102]) for k, v in want.items()}
    same(K_.triangulate_keypoints(K[:, :102].reshape(7, 2, 3, 17, 3), cams[:, :6].reshape(7, 2, 3, 21), view_residual=True), six, (2, 3, 17))
    one = K_.triangulate_keypoints(K[:, :17], np.ascontiguousarray(cams[:, 0]))                   # a single frame [C,17,3] with a static rig
    assert one.points.shape == (17, 3) and one.state.shape == (17,)
    assert np.array_equal(raw(one.points), raw(want["points"][:17]))
    empty = K_.triangulate_keypoints(K[:, :0].reshape(7, 0, 17, 3), np.ascontiguousarray(cams[:, 0]), view_residual=True)
    assert empty.points.shape == (0, 17, 3) and empty.view_residual.shape == (7, 0, 17) and empty.points.is_cuda


def test_a_frame_alone_equals_the_frame_in_the_batch(cases):
    import kasportsformer_amd as K_
    K, cams, want = cases[31, 16]
    K5 = K.reshape(16, 31, 17, 3)
    full = K_.triangulate_keypoints(K5, cams, view_residual=True)
    for f in (0, 7, 8, 30):                                                                       # frames 7 and 8 straddle the first tile's end at point 128
        one = K_.triangulate_keypoints(K5[:, f:f + 1], cams[:, f:f + 1], view_residual=True)
        for name in FIELDS:
            part = getattr(full, name)[:, f:f + 1] if name == "view_residual" else getattr(full, name)[f:f + 1]
            assert np.array_equal(raw(getattr(one, name)), raw(part)), (f, name)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("key", [(241, 7), (15, 16)])
def test_the_entry_writes_nothing_else_and_takes_null_outputs(cases, offset, key):
    """The C entry with sentinels around every output, at 16-byte aligned pointers and at pointers 4 bytes past them, static (241 frames) and per-frame (15)
    cameras; then each optional output NULL in turn."""
    from kasportsformer_amd import _lib
    K, cams, want = cases[key]
    views, M = K.shape[:2]
    lib = _lib.load()
    buf = torch.zeros(K.size + 8, device="cuda")
    buf[offset:offset + K.size] = torch.from_numpy(K.reshape(-1)).cuda()
    Kd, cd = buf[offset:offset + K.size], torch.from_numpy(cams).cuda()
    q = _lib.KasfTriangulateParams(0.3, 1, 4, 3.0, 2, 5)
    sizes = {"points": M * 3, "residual": M, "used": M, "state": M, "view_residual": views * M}
    for null in (None, "residual", "used", "state", "view_residual"):
        bufs = {k: torch.full((n + 128 + offset,), 77 if k in BYTES else CAN, dtype=torch.uint8 if k in BYTES else torch.float32, device="cuda")
                for k, n in sizes.items()}
        lo = {k: 64 + (offset if k in ("points", "view_residual") else 0) for k in sizes}
        view = {k: bufs[k][lo[k]:lo[k] + n] for k, n in sizes.items()}
        arg = lambda k: None if k == null else ptr(view[k])             # noqa: E731
        _lib.check(lib.kasf_keypoints_triangulate(ptr(Kd), views, M, 17, ptr(cd), int(cams.ndim == 3), C.byref(q), arg("points"), arg("residual"), arg("used"),
                                                  arg("state"), arg("view_residual"), stream()))
        for k, n in sizes.items():
            fill = 77 if k in BYTES else CAN
            assert (bufs[k][:lo[k]] == fill).all() and (bufs[k][lo[k] + n:] == fill).all(), (null, k)
            if k == null:
                assert (view[k] == fill).all()
            else:
                assert np.array_equal(raw(view[k]), raw(want[k]).reshape(-1)), (null, k)
    assert np.array_equal(raw(Kd), raw(K.reshape(-1))) and np.array_equal(raw(cd), raw(cams))


@pytest.mark.parametrize("points,joints,rounds", [(1, 1, 5), (255, 1, 5), (256, 1, 0), (257, 1, 20), (513, 1, 5), (31 * 17, 17, 5)])
def test_undistort_keypoints_equals_the_restatement_bit_for_bit(points, joints, rounds):
    import kasportsformer_amd as K_
    frames = points // joints
    per_frame = frames % 2 == 1 and frames > 1
    K, cams, _ = bundle(frames, 3, seed=points, per_frame=per_frame, distortion=LENS, joints=joints)
    kp = K[1].copy()
    kp[::50, 1] = np.inf                                                                          # not usable: copied as it came
    cam9 = np.ascontiguousarray(cams[1, ..., :9])
    want = undistort_np(kp, cam9, joints, rounds).reshape(frames, joints, 3)
    kp3 = kp.reshape(frames, joints, 3)
    kd = torch.from_numpy(kp3).cuda()
    got = K_.undistort_keypoints(kd, torch.from_numpy(cam9[..., :4].copy()).cuda(), torch.from_numpy(cam9[..., 4:].copy()).cuda(), iterations=rounds)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(raw(got), raw(want)) and np.array_equal(raw(kd), raw(kp3))
    again = K_.undistort_keypoints(kp3, cam9[..., :4].copy(), cam9[..., 4:].copy(), iterations=rounds)                # from the host, a second run
    assert np.array_equal(raw(again), raw(want))
    if per_frame:                                                                                 # one lens for every frame of a zooming camera
        mixed = K_.undistort_keypoints(kp3, cam9[:, :4].copy(), cam9[0, 4:].copy(), iterations=rounds)
        assert np.array_equal(raw(mixed), raw(want))


@pytest.mark.parametrize("offset", [0, 1])
def test_the_undistort_entry_writes_nothing_else(offset):
    from kasportsformer_amd import _lib
    K, cams, _ = bundle(513, 3, seed=9, distortion=LENS, joints=1)
    kp, cam9 = K[2], np.ascontiguousarray(cams[2, :9])
    want = undistort_np(kp, cam9, 1, 5)
    src = torch.zeros(kp.size + 8, device="cuda")
    src[offset:offset + kp.size] = torch.from_numpy(kp.reshape(-1)).cuda()
    dst = torch.full((kp.size + 128 + offset,), CAN, device="cuda")
    out = dst[64 + offset:64 + offset + kp.size]
    _lib.check(_lib.load().kasf_keypoints_undistort(ptr(src[offset:]), 513, 1, ptr(torch.from_numpy(cam9).cuda()), 0, 5, ptr(out), stream()))
    assert (dst[:64 + offset] == CAN).all() and (dst[64 + offset + kp.size:] == CAN).all()
    assert np.array_equal(raw(out), raw(want.reshape(-1))) and np.array_equal(raw(src[offset:offset + kp.size]), raw(kp.reshape(-1)))


def test_points_that_are_not_triangulated_are_filled_by_refine_tracks():
    import kasportsformer_amd as K_
    from tests.triangulate_ref import project, ring
    n, views = 120, 4
    cams = ring(views, distortion=LENS)
    t = np.linspace(0.0, 1.0, n)
    centre = np.stack([-3.0 + 6.0 * t, 1.0 - 2.0 * t, np.ones(n)], 1)
    X = (centre[:, None, :] + np.random.default_rng(8).uniform(-0.8, 0.8, (1, 17, 3))).reshape(-1, 3)
    K = np.concatenate([project(X, cams), np.full((views, n * 17, 1), 0.9)], -1).astype(np.float32).reshape(views, n, 17, 3)
    lost = (np.arange(n) % 17 == 5) | ((np.arange(n) >= 60) & (np.arange(n) < 66))
    K[1:, lost, :, 2] = 0.0                                                                       # one camera left: too few views
    r = K_.triangulate_keypoints(K, cams)
    assert np.array_equal((r.state.cpu().numpy() != 0).all(1), lost) and np.array_equal((r.state.cpu().numpy() == 1).any(1), lost)
    assert torch.isnan(r.points[torch.from_numpy(lost).cuda()]).all()
    joints, st = K_.refine_tracks(r.points, score=False, return_state=True)
    assert torch.isfinite(joints).all() and np.array_equal((st.cpu().numpy() == 1).all(1), lost)
    assert np.abs(joints.cpu().numpy().astype(np.float64).reshape(-1, 3) - X).max() < 2e-3


def test_undistorted_keypoints_place_a_pose_where_the_lens_model_saw_it():
    """The chain the command line's --camera-distortion runs: undistort_keypoints in front of place_poses puts the root where the player stood; the distorted
    keypoints put it elsewhere."""
    import kasportsformer_amd as K_
    from tests.place_ref import scene
    from tests.triangulate_ref import project
    P, T, _, camera = scene(np.random.default_rng(3), 64, depth=(4.0, 12.0))
    cam = np.concatenate([camera, LENS, np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
    X = (P.astype(np.float64) + T[:, None, :]).reshape(-1, 3)
    kp = np.concatenate([project(X, cam[None])[0], np.full((len(X), 1), 0.9)], -1).astype(np.float32).reshape(64, 17, 3)
    good = K_.place_poses(P, K_.undistort_keypoints(kp, camera, LENS), camera)
    bad = K_.place_poses(P, kp, camera)
    err = lambda r: np.linalg.norm(r.root.cpu().numpy().astype(np.float64) - T, axis=1)           # noqa: E731
    assert (good.state == 0).all() and np.median(err(good)) < 1e-3 and np.median(err(bad)) > 20 * np.median(err(good))
