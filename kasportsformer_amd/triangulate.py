"""From several cameras: one player's keypoint tracks in C calibrated cameras triangulated to joints in the world frame, and the lens undistortion, on the device.

    cams = np.stack([camera_row((fx, fy, cx, cy), (k1, k2, p1, p2, k3), R, t) for ...])   # [C,21]; X_cam = R X_world + t
    r = triangulate_keypoints([kp_cam0, kp_cam1, ...], cams)        # each [N,17,3] pixel x, pixel y, score -> r.points [N,17,3] in the world frame
    r.points, r.residual, r.used, r.state, r.view_residual          # [...,J,3], [...,J] float32 (pixels), [...,J] uint8, [...,J] uint8, [C,...,J] or None
    joints = refine_tracks(r.points, score=False)                   # recorded: points that could not be triangulated are NaN and are interpolated here
    kp_u = undistort_keypoints(kp, (fx, fy, cx, cy), (k1, k2, p1, p2, k3))                 # pixels in, undistorted pixels out: what place_poses wants

include/kasf.h (``kasf_keypoints_triangulate``) states the camera model and the rule in full, once.  A camera is 21 float32 values: fx, fy, cx, cy in pixels,
the Brown-Conrady coefficients k1, k2, p1, p2, k3 in OpenCV's order, R row-major and t.  Per point -- one joint of one frame -- a view is usable by the One-Euro
filter's test (finite keypoint, score at least ``min_score``) when its camera's values are finite; its keypoint is undistorted by ``undistort_iterations``
rounds of a fixed-point iteration (0: a pinhole); the usable views' rays give a 3 x 3 weighted least-squares problem, accumulated and solved in fp64;
``iterations`` rounds re-weight it to pixels at the point's depth with a Cauchy weight of ``delta`` pixels, which takes a view that does not fit -- a swapped
joint -- out when three or more views see the point (with two, nothing tells which one is wrong: only ``residual`` shows it).  Results are rounded to fp32 once.

``state`` per point: 0 triangulated; 1 fewer than ``min_views`` usable views; 2 degenerate (rays that do not spread, a result that is not finite); 3 behind a
usable camera.  A point whose state is not 0 is NaN in ``points``, ``residual`` and ``view_residual``, so that ``refine_tracks(points, score=False)`` over a
recorded track fills it.  ``residual``: the weighted RMS re-projection error in pixels of the undistorted images; ``view_residual``: the error per view -- what
to check a lifted and placed pose against, and what tells which camera's calibration has drifted.  Points are independent: a recorded track and one live tick
are the same call.  One launch, nothing read back, no host path.

Not here: calibration itself (estimating R, t or the coefficients), temporal synchronisation of the cameras, moving cameras for the matching
in front of this call (``match_players`` says which rows of which cameras are ONE player: a static rig, no stateful live matcher that keeps group ids from tick to
tick, no cycle-consistent multi-way matching), rational and fisheye lens models, bundle adjustment.  The defaults are a starting point, not tuned on footage; accuracy has been shown
on synthetic players only.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in, number

MIN_VIEWS, MAX_VIEWS, MAX_ITERATIONS, MAX_ROUNDS, CAMERA_FLOATS = 2, 16, 8, 20, 21


class TriangulateResult(NamedTuple):
    """What ``triangulate_keypoints`` returns, all on the device: ``points`` [...,J,3] and ``residual`` [...,J] (pixels) float32, ``used`` [...,J] uint8 (usable
    views), ``state`` [...,J] uint8 (0 triangulated, 1 too few views, 2 degenerate, 3 behind a camera), ``view_residual`` [C,...,J] float32 or None."""
    points: torch.Tensor
    residual: torch.Tensor
    used: torch.Tensor
    state: torch.Tensor
    view_residual: Optional[torch.Tensor]


def camera_row(intrinsics, distortion, R, t) -> np.ndarray:
    """The 21 values of a camera as ``triangulate_keypoints`` takes them: ``intrinsics`` (fx, fy, cx, cy) in pixels, ``distortion`` (k1, k2, p1, p2, k3) or None
    for a pinhole, ``R`` [3,3] and ``t`` [3] with X_cam = R X_world + t -> float32 [21].  Leading dimensions (a row per frame) are carried through."""
    who = "camera_row"
    k = np.asarray(intrinsics, np.float32)
    d = np.zeros(k.shape[:-1] + (5,), np.float32) if distortion is None else np.asarray(distortion, np.float32)
    R, t = np.asarray(R, np.float32), np.asarray(t, np.float32)
    lead = k.shape[:-1]
    if k.shape[-1:] != (4,) or d.shape != lead + (5,) or R.shape != lead + (3, 3) or t.shape != lead + (3,):
        raise ValueError(f"{who}: expected intrinsics [...,4], distortion [...,5], R [...,3,3] and t [...,3] with the same leading shape, got {k.shape}, {d.shape}, "
                         f"{R.shape} and {t.shape}")
    return np.concatenate([k, d, R.reshape(lead + (9,)), t], -1)        # a row with a value that is not finite marks its view as not usable


def triangulate_params(min_score=0.3, weighted=True, iterations=4, delta=3.0, min_views=2, undistort_iterations=5,
                       who: str = "triangulate_keypoints") -> _lib.KasfTriangulateParams:
    """The parameters as the entry point takes them, refused as the entry point refuses them."""
    min_score, delta = number(min_score, who, "min_score"), number(delta, who, "delta")
    if not np.float32(delta) > 0:
        raise ValueError(f"{who}: delta must be > 0 pixels, got {delta}")
    if not isinstance(weighted, (bool, np.bool_)):
        raise TypeError(f"{who}: weighted must be a bool, got {type(weighted).__name__}")
    iterations = index_in(iterations, who, "iterations", 0, MAX_ITERATIONS)
    min_views = index_in(min_views, who, "min_views", MIN_VIEWS, MAX_VIEWS)
    undistort_iterations = index_in(undistort_iterations, who, "undistort_iterations", 0, MAX_ROUNDS)
    return _lib.KasfTriangulateParams(min_score, int(weighted), iterations, delta, min_views, undistort_iterations)


def triangulate_keypoints(keypoints, cameras, *, min_score: float = 0.3, weighted: bool = True, iterations: int = 4, delta: float = 3.0, min_views: int = 2,
                          undistort_iterations: int = 5, view_residual: bool = False, device=None) -> TriangulateResult:
    """One player's keypoints in C cameras -> joints in the world frame; see the module docstring.  ``keypoints``: [C,...,J,3] (pixel x, pixel y, score), or a
    list of C arrays [...,J,3] of one shape, 2 <= C <= 16: float32, numpy or torch, on the host or the GPU, never modified.  ``cameras``: float32 [C,21]
    (``camera_row``) for a static rig, or ``[C] + keypoints.shape[1:-2] + [21]``, a row per camera and frame, for moving cameras.  ``min_score``: a keypoint
    scored below it is not used; ``weighted``: weigh a view by its score; ``iterations`` in [0, 8] rounds of re-weighting with ``delta`` pixels; ``min_views`` in
    [2, 16]; ``undistort_iterations`` in [0, 20] (0: a pinhole); ``view_residual``: also return the error per view.  -> ``TriangulateResult`` on the device; a
    point whose ``state`` is not 0 is NaN in ``points``, ``residual`` and ``view_residual``.  One launch.  Every refusal is raised before any launch."""
    who = "triangulate_keypoints"
    params = triangulate_params(min_score, weighted, iterations, delta, min_views, undistort_iterations, who)
    if not isinstance(view_residual, (bool, np.bool_)):
        raise TypeError(f"{who}: view_residual must be a bool, got {type(view_residual).__name__}")
    if isinstance(keypoints, (list, tuple)):
        parts = [_args.as_tensor(a, who, f"keypoints[{i}]", _args.FLOAT32) for i, a in enumerate(keypoints)]
        if not MIN_VIEWS <= len(parts) <= MAX_VIEWS:
            raise ValueError(f"{who}: expected the keypoints of 2 to 16 cameras, got {len(parts)}")
        if any(tuple(p.shape) != tuple(parts[0].shape) for p in parts):
            raise ValueError(f"{who}: every camera's keypoints must have one shape, got {[tuple(p.shape) for p in parts]}")
    else:
        parts = None
        k = _args.as_tensor(keypoints, who, "keypoints", _args.FLOAT32)
    shape = ((len(parts),) + tuple(parts[0].shape)) if parts is not None else tuple(k.shape)
    if len(shape) < 3 or shape[-1] != 3 or shape[-2] < 1:
        raise ValueError(f"{who}: expected keypoints of [C,...,J,3] with J >= 1, got {shape}")
    if not MIN_VIEWS <= shape[0] <= MAX_VIEWS:
        raise ValueError(f"{who}: expected the keypoints of 2 to 16 cameras, got {shape[0]}")
    views, lead, J = shape[0], shape[1:-2], shape[-2]
    cam = _args.as_tensor(cameras, who, "cameras", _args.FLOAT32)
    if tuple(cam.shape) == (views, CAMERA_FLOATS):
        cam_rows = False
    elif len(lead) > 0 and tuple(cam.shape) == (views,) + lead + (CAMERA_FLOATS,):
        cam_rows = True
    else:
        raise ValueError(f"{who}: cameras must be [{views}, 21] (fx, fy, cx, cy, k1, k2, p1, p2, k3, R, t) or {[views] + list(lead) + [21]}, one row per camera "
                         f"and frame, got {tuple(cam.shape)}")
    dev = _args.resolve_device((parts if parts is not None else [k]) + [cam], device, who)
    k = torch.stack([p.to(dev) for p in parts]) if parts is not None else k.to(dev)
    k, cam = k.contiguous(), cam.to(dev).contiguous()
    M = int(np.prod(lead, dtype=np.int64)) * J
    points = torch.empty(lead + (J, 3), dtype=torch.float32, device=dev)
    residual = torch.empty(lead + (J,), dtype=torch.float32, device=dev)
    used, state = torch.empty(lead + (J,), dtype=torch.uint8, device=dev), torch.empty(lead + (J,), dtype=torch.uint8, device=dev)
    per_view = torch.empty((views,) + lead + (J,), dtype=torch.float32, device=dev) if view_residual else None
    if M > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kasf_keypoints_triangulate(k.data_ptr(), views, M, J, cam.data_ptr(), int(cam_rows), C.byref(params), points.data_ptr(),
                                                              residual.data_ptr(), used.data_ptr(), state.data_ptr(),
                                                              per_view.data_ptr() if per_view is not None else None, _args.stream()))
    return TriangulateResult(points, residual, used, state, per_view)


def _lens_rows(a, who: str, name: str, lead, width: int, what: str):
    t = _args.as_tensor(a, who, name, _args.FLOAT32)
    if tuple(t.shape) == (width,):
        return t, False
    if len(lead) > 0 and tuple(t.shape) == tuple(lead) + (width,):
        return t, True
    raise ValueError(f"{who}: {name} must be [{width}] ({what}) or {list(lead) + [width]}, one row per frame, got {tuple(t.shape)}")


def undistort_keypoints(keypoints, camera, distortion, *, iterations: int = 5, device=None) -> torch.Tensor:
    """Keypoints of a lens with Brown-Conrady distortion -> the keypoints an ideal pinhole with the same intrinsics would have seen: what ``place_poses`` and any
    pinhole geometry want.  ``keypoints`` [...,J,3] (pixel x, pixel y, score): float32, numpy or torch, on the host or the GPU, never modified.  ``camera``:
    float32 [4] = fx, fy, cx, cy, or ``keypoints.shape[:-2] + (4,)``, a row per frame; ``distortion``: float32 [5] = k1, k2, p1, p2, k3 (OpenCV's order), or a
    row per frame.  ``iterations`` in [0, 20] rounds of the fixed-point iteration of include/kasf.h (five come within 2e-4 px for a wide action-camera lens).
    -> float32 [...,J,3] on the device; the score is copied, and so is a keypoint that is not finite.  One launch.  Every refusal is raised before any launch."""
    who = "undistort_keypoints"
    iterations = index_in(iterations, who, "iterations", 0, MAX_ROUNDS)
    k = _args.as_tensor(keypoints, who, "keypoints", _args.FLOAT32)
    if k.dim() < 2 or k.shape[-1] != 3 or k.shape[-2] < 1:
        raise ValueError(f"{who}: expected keypoints of [...,J,3] with J >= 1, got {tuple(k.shape)}")
    lead, J = tuple(k.shape[:-2]), int(k.shape[-2])
    cam, cam_rows = _lens_rows(camera, who, "camera", lead, 4, "fx, fy, cx, cy")
    lens, lens_rows = _lens_rows(distortion, who, "distortion", lead, 5, "k1, k2, p1, p2, k3")
    dev = _args.resolve_device([k, cam, lens], device, who)
    k, cam, lens = k.to(dev).contiguous(), cam.to(dev), lens.to(dev)
    rows = cam_rows or lens_rows
    if rows:
        cam, lens = cam.expand(lead + (4,)), lens.expand(lead + (5,))
    row9 = torch.cat([cam, lens], -1).contiguous()
    M = int(np.prod(lead, dtype=np.int64)) * J
    out = torch.empty_like(k)
    if M > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kasf_keypoints_undistort(k.data_ptr(), M, J, row9.data_ptr(), int(rows), iterations, out.data_ptr(), _args.stream()))
    return out
