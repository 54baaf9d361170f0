"""Where each player stands: lifted poses placed in camera space from their 2-D keypoints and the camera's intrinsics, on the device.

    r = place_poses(out.poses, kp, camera)                          # live: behind lifter.push(kp, t); camera = (fx, fy, cx, cy) in pixels
    r = place_poses(poses, keypoints, camera, metric_lengths=table) # poses in the model's unit, roots in metres: a bone table [16] in metres
    r.poses, r.root, r.residual, r.scale, r.state                   # [...,17,3], [...,3], [...], [...] float32 and [...] uint8, all on the device
    roots = refine_tracks(r.root.unsqueeze(-2), score=False)        # recorded: frames that could not be placed are NaN and are interpolated here
    world = poses_to_world(r.poses, rotation, translation)          # the camera's extrinsics, then poses_to_panel / draw_poses

The lifters return every pose root-relative, joint 0 at the origin, so ``poses_to_panel`` and ``draw_poses`` paint a team on one spot.  The root translation
that makes a pose re-project onto the keypoints it was lifted from is a 3 x 3 weighted least-squares problem per frame; include/kasf.h (``kasf_pose_place``)
states the rule in full: a joint is usable by the One-Euro filter's test (finite keypoint, score at least ``min_score``) when its pose values are finite;
the fit is accumulated and solved in fp64 (the system's condition number reaches 4e4 for players at 40 m); ``iterations`` rounds of Cauchy re-weighting with
``delta`` pixels take the weight off a keypoint that does not fit, a swapped wrist for instance; results are rounded to fp32 once.  The camera is a pinhole:
for a lens with distortion, send the keypoints through ``undistort_keypoints`` (triangulate.py) first.

Metres come one of two ways.  ``metric_lengths``: a table of the sixteen bone lengths in metres (``bones.BONE_PARENTS``' bones, 0 skips a bone); every frame's
pose is multiplied by (the table's sum) / (the frame's sum over the same bones) before the fit -- per frame, because the model's unit is image pixels and a
player's size in it changes with depth.  Or ``fix_bone_lengths(poses, lengths=table)`` first, which makes the poses metric bone by bone, and no table here.

``state`` per frame: 0 placed; 1 fewer than ``min_joints`` usable joints; 2 a degenerate fit (keypoints that do not spread, a solution that is not finite or
puts a usable joint behind the camera); 3 a scale that is not finite and positive.  A frame whose state is not 0 gets NaN in ``poses``, ``root`` and
``residual``, so that ``refine_tracks(..., score=False)`` over a recorded track interpolates it from its neighbours.  Frames are independent: a recorded track
and one live tick are the same call.  One launch, nothing read back, no host path.  The defaults are a starting point, not tuned on footage; accuracy has been
shown on synthetic players only.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in, number as _number

MAX_ITERATIONS, MIN_JOINTS, JOINTS, BONES = 8, 2, 17, 16       # iterations in [0, 8] and min_joints in [2, 17] of kasf_pose_place


class PlaceResult(NamedTuple):
    """What ``place_poses`` returns, all on the device: ``poses`` [...,17,3], ``root`` [...,3], ``residual`` [...] (pixels) and ``scale`` [...] float32,
    ``state`` [...] uint8 (0 placed, 1 too few joints, 2 degenerate fit, 3 scale not usable)."""
    poses: torch.Tensor
    root: torch.Tensor
    residual: torch.Tensor
    scale: torch.Tensor
    state: torch.Tensor


def place_params(min_score=0.3, weighted=True, iterations=4, delta=3.0, min_joints=4, who: str = "place_poses") -> _lib.KasfPlaceParams:
    """The parameters as the entry point takes them, refused as the entry point refuses them."""
    min_score, delta = _number(min_score, who, "min_score"), _number(delta, who, "delta")
    if not np.float32(delta) > 0:
        raise ValueError(f"{who}: delta must be > 0 pixels, got {delta}")
    if not isinstance(weighted, (bool, np.bool_)):
        raise TypeError(f"{who}: weighted must be a bool, got {type(weighted).__name__}")
    iterations = index_in(iterations, who, "iterations", 0, MAX_ITERATIONS)
    min_joints = index_in(min_joints, who, "min_joints", MIN_JOINTS, JOINTS)
    return _lib.KasfPlaceParams(min_score, int(weighted), iterations, delta, min_joints)


def load_bone_table(path: str) -> np.ndarray:
    """``python -m kasportsformer_amd.lift --place-lengths``: an ``.npy`` (no pickles) of sixteen finite bone lengths >= 0 in metres, at least one of them > 0 -> float32 [16]."""
    t = np.load(path, allow_pickle=False)
    if t.shape != (16,) or not np.issubdtype(t.dtype, np.number) or np.iscomplexobj(t):
        raise ValueError(f"{path}: expected sixteen bone lengths [16], got {t.dtype} {t.shape}")
    t = t.astype(np.float32)
    if not (np.isfinite(t).all() and (t >= 0).all() and (t > 0).any()):
        raise ValueError(f"{path}: the bone lengths must be finite, >= 0 (0 skips a bone) and not all 0")
    return t


def _rows(a, who: str, name: str, lead, width: int, what: str):
    """``camera`` / ``metric_lengths``: float32 [width], or lead + (width,) -> (the tensor where it is, whether it has a row per frame)."""
    t = _args.as_tensor(a, who, name, _args.FLOAT32)
    if tuple(t.shape) == (width,):
        return t, False
    if tuple(t.shape) != tuple(lead) + (width,):
        raise ValueError(f"{who}: {name} must be [{width}] ({what}) or {list(lead) + [width]}, one row per frame, got {tuple(t.shape)}")
    return t, True


def place_poses(poses, keypoints, camera, *, metric_lengths=None, min_score: float = 0.3, weighted: bool = True, iterations: int = 4, delta: float = 3.0,
                min_joints: int = 4, device=None) -> PlaceResult:
    """Root-relative poses placed in front of the camera; see the module docstring.  ``poses`` [...,17,3] (any one unit) and ``keypoints`` of the same shape
    (pixel x, pixel y, score in the H36M-17 layout): float32, numpy or torch, on the host or the GPU, never modified.  ``camera``: float32 [4] = fx, fy, cx, cy
    in pixels (a pinhole: ``undistort_keypoints`` goes in front for a lens), or ``poses.shape[:-2] + (4,)``, a row per frame.  ``metric_lengths``: None, or float32 [16] metres (0 skips a bone), or
    ``poses.shape[:-2] + (16,)``.  ``min_score``: a keypoint scored below it is not used; ``weighted``: weigh a keypoint by its score; ``iterations`` in [0, 8]
    rounds of Cauchy re-weighting with ``delta`` pixels; ``min_joints`` in [2, 17].  -> ``PlaceResult`` on the device; a frame whose ``state`` is not 0 is NaN in
    ``poses``, ``root`` and ``residual`` (``refine_tracks(r.root.unsqueeze(-2), score=False)`` fills it on a recorded track).  One launch.  The defaults are a
    starting point, not tuned on footage.  Every refusal is raised before any launch."""
    who = "place_poses"
    params = place_params(min_score, weighted, iterations, delta, min_joints, who)
    p = _args.as_tensor(poses, who, "poses", _args.FLOAT32)
    k = _args.as_tensor(keypoints, who, "keypoints", _args.FLOAT32)
    if p.dim() < 2 or tuple(p.shape[-2:]) != (JOINTS, 3):
        raise ValueError(f"{who}: expected poses of [...,17,3], got {tuple(p.shape)}")
    if tuple(k.shape) != tuple(p.shape):
        raise ValueError(f"{who}: keypoints must have the poses' shape {tuple(p.shape)} (pixel x, pixel y, score), got {tuple(k.shape)}")
    lead = tuple(p.shape[:-2])
    cam, cam_rows = _rows(camera, who, "camera", lead, 4, "fx, fy, cx, cy")
    table, table_rows = _rows(metric_lengths, who, "metric_lengths", lead, BONES, "metres per bone") if metric_lengths is not None else (None, False)
    dev = _args.resolve_device([p, k, cam, table], device, who)
    frames = int(np.prod(lead, dtype=np.int64))
    p, k, cam = p.to(dev).contiguous(), k.to(dev).contiguous(), cam.to(dev).contiguous()
    table = table.to(dev).contiguous() if table is not None else None
    out = torch.empty(lead + (JOINTS, 3), dtype=torch.float32, device=dev)
    root = torch.empty(lead + (3,), dtype=torch.float32, device=dev)
    residual, scale = torch.empty(lead, dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.float32, device=dev)
    state = torch.empty(lead, dtype=torch.uint8, device=dev)
    if frames > 0:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kasf_pose_place(p.data_ptr(), k.data_ptr(), frames, cam.data_ptr(), int(cam_rows), table.data_ptr() if table is not None else None,
                                                   int(table_rows), C.byref(params), out.data_ptr(), root.data_ptr(), residual.data_ptr(), scale.data_ptr(),
                                                   state.data_ptr(), _args.stream()))
    return PlaceResult(out, root, residual, scale, state)
