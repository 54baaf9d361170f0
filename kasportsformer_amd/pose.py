"""The two ends of the lift that the demo does on the host, on the GPU: what a 2-D detector writes in, what the demo plots out.

    kp = coco_to_h36m(coco)                                      # [...,17,3] COCO-17 pixel x, y, score -> CUDA fp32 [...,17,3] in the H36M-17 layout
    kp = coco_to_h36m(keypoints, scores)                         # [...,17,2] + [...,17]: the pair ``gen_video_kpts`` returns
    world = poses_to_world(poses, floor=True, unit=True)         # the lift's camera-space poses -> what demo.py:242-248 plots

``coco_to_h36m`` is ``h36m_coco_format`` (demo/lib/preprocess.py:10-69, applied to the HRNet output in demo/demo.py:75-78): every off-the-shelf 2-D pose
model (YOLO-pose, RTMPose, ViTPose, the demo's HRNet) emits COCO-17 with per-joint scores, the model was trained on Human3.6M's 17 joints.  Bit for bit the
reference's keypoints and scores, with one difference: shapes are kept.  The reference drops a whole person whose coordinates sum to exactly zero; here a
frame of zeros converts to a frame of zeros.  ``layout="coco"`` on ``lift_track``, ``lift_tracks`` and ``StreamLifter`` runs it in front of the lift.

``poses_to_world`` is ``camera_to_world`` (demo/lib/utils.py:55-73) and, on request, the two lines after it in the demo: feet on the floor, unit scale.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _args, _lib

LAYOUTS = ("h36m", "coco")
# demo/demo.py:243: the camera rotation the demo views every clip with, a unit quaternion (w, x, y, z)
DEMO_CAMERA_ROTATION = (0.1407056450843811, -0.1500701755285263, -0.755240797996521, 0.6223280429840088)


def check_layout(layout, who: str) -> bool:
    """``layout=`` of a lift surface -> whether the keypoints are COCO-17; anything but "h36m" / "coco" raises ``ValueError``."""
    if layout not in LAYOUTS:
        raise ValueError(f"{who}: layout must be one of {LAYOUTS}, got {layout!r}")
    return layout == "coco"


def convert_frames(frames: torch.Tensor) -> torch.Tensor:
    """``kasf_coco_h36m`` on a contiguous CUDA fp32 [...,17,3] tensor: a new tensor of its shape (what the lift surfaces call with ``layout="coco"``)."""
    out = torch.empty_like(frames)
    n = frames.numel() // 51
    if n:
        with torch.cuda.device(frames.device):
            _lib.check(_lib.load().kasf_coco_h36m(frames.data_ptr(), n, out.data_ptr(), _args.stream()))
    return out


def coco_to_h36m(keypoints, scores=None, device=None) -> torch.Tensor:
    """COCO-17 detector keypoints -> the H36M-17 layout ``lift_track`` / ``lift_tracks`` / ``StreamLifter`` take: ``keypoints`` [...,17,3] (pixel x,
    pixel y, score), or [...,17,2] with ``scores`` [...,17] (what ``gen_video_kpts`` returns); float32, numpy or torch, CPU or GPU, never modified ->
    CUDA fp32 [...,17,3].  Coordinates as ``coco_h36m`` (demo/lib/preprocess.py:10-37), scores as ``h36m_coco_format`` (:58-62), bit for bit; a frame
    of zeros stays a frame of zeros (the reference drops an all-zero person).  ``device``: where host input goes (default: the current GPU); GPU input
    stays where it is.  There is no host path: without a GPU the call raises ``RuntimeError``.  Exception types as ``lift_tracks``."""
    who = "coco_to_h36m"
    kp = _args.as_tensor(keypoints, who, "keypoints", _args.FLOAT32)
    if scores is None:
        if kp.dim() < 2 or tuple(kp.shape[-2:]) != (17, 3):
            raise ValueError(f"{who}: expected keypoints [...,17,3] (or [...,17,2] with scores [...,17]), got {tuple(kp.shape)}")
        sc = None
    else:
        sc = _args.as_tensor(scores, who, "scores", _args.FLOAT32)
        if kp.dim() < 2 or tuple(kp.shape[-2:]) != (17, 2) or tuple(sc.shape) != tuple(kp.shape[:-1]):
            raise ValueError(f"{who}: expected keypoints [...,17,2] and scores [...,17], got {tuple(kp.shape)} and {tuple(sc.shape)}")
    dev = _args.resolve_device((kp, sc), device, who)
    if sc is None:
        frames = kp.to(dev).contiguous()                     # a copy when it comes from the host; on the device the kernel only reads it
    else:
        frames = torch.cat((kp.to(dev), sc.to(dev).unsqueeze(-1)), dim=-1)
    return convert_frames(frames)


def _vector(value, n: int, who: str, name: str) -> np.ndarray:
    v = np.asarray(value.detach().cpu() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
    if v.ndim == 0 and name == "translation":
        v = np.full(n, v)
    if v.shape != (n,) or not np.all(np.isfinite(v)):
        raise ValueError(f"{who}: {name} must be {n} finite numbers, got {value!r}")
    return np.ascontiguousarray(v, dtype=np.float32)


def poses_to_world(poses, rotation=DEMO_CAMERA_ROTATION, translation=0.0, floor: bool = False, unit: bool = False) -> torch.Tensor:
    """Camera-space poses -> world space: ``poses`` CUDA fp32 [...,17,3] (the lifts' output; never modified) -> a new tensor of its shape.  Every joint
    v becomes ``v + 2 * (q0 * (q x v) + q x (q x v)) + t`` in fp32 with ``qrot``'s operation order (``camera_to_world``, demo/lib/utils.py:55-73);
    ``rotation`` is the quaternion (w, x, y, z), by default the demo's (demo.py:243), ``translation`` one number or three.  ``floor``: the smallest z of
    each frame is subtracted from its z column (demo.py:246).  ``unit``: all 51 values of each frame are divided by their largest (demo.py:247-248),
    after the floor step when both are set.  A degenerate frame whose largest value is 0 gets what the reference's division gives (inf / nan): it is
    not guarded.  On its own the call is the rotation (and translation) only."""
    who = "poses_to_world"
    if not isinstance(poses, torch.Tensor):
        raise TypeError(f"{who}: poses must be a CUDA torch tensor, got {type(poses).__name__}")
    if poses.dtype != torch.float32:
        raise TypeError(f"{who}: poses must be float32, got {poses.dtype}")
    if not poses.is_cuda:
        raise RuntimeError(f"{who}: poses must be on the GPU, got {poses.device}; kasportsformer_amd has no CPU path")
    if poses.dim() < 2 or tuple(poses.shape[-2:]) != (17, 3):
        raise ValueError(f"{who}: expected poses [...,17,3], got {tuple(poses.shape)}")
    q, t = _vector(rotation, 4, who, "rotation"), _vector(translation, 3, who, "translation")
    src = poses.detach().contiguous()
    out = torch.empty_like(src)
    n = src.numel() // 51
    if n:
        with torch.cuda.device(src.device):
            _lib.check(_lib.load().kasf_pose_world(src.data_ptr(), n, q.ctypes.data, t.ctypes.data, int(bool(floor)), int(bool(unit)), out.data_ptr(),
                                                   _args.stream()))
    return out
