"""The step in front of ``coco_to_h36m``: a top-down pose network's heatmaps decoded to keypoints on the GPU they were computed on.

    kp = heatmaps_to_keypoints(hm, center, scale)                         # hm [...,17,H,W] on the GPU -> CUDA fp32 [...,17,3] COCO-17 image x, y, score
    kp = heatmaps_to_keypoints(hm, boxes=boxes, aspect=frame_h / frame_w) # the detector's boxes instead of the crop's center / scale
    kp = heatmaps_to_keypoints(hm, center, scale, layout="h36m")          # ... and through coco_to_h36m: what lift_track / lift_tracks take
    poses = lifter.push_heatmaps(hm, center, scale)                       # StreamLifter: decode, then push

``heatmaps_to_keypoints`` is ``get_final_preds`` (demo/lib/hrnet/lib/utils/inference.py:21-82: argmax per joint map, the quarter-pixel ``POST_PROCESS``
step, ``transform_preds`` back to image pixels), which the demo runs on the host on a copy of HRNet's output (demo/lib/hrnet/gen_kpts.py:158-161); HRNet,
ViTPose and SimpleBaseline all end in it.  Positions, scores and refined heatmap coordinates are the reference's bit for bit; the image coordinates are the
closed form of its three-point affine evaluated in fp64 and rounded once, within 1 fp32 ulp of what the reference's ``cv2.getAffineTransform`` solve
gives (include/kasf.h, ``kasf_heatmap_keypoints``, states every rule).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .pose import _float32, _stream, check_layout

_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}
_NP_DTYPES = (np.float32, np.float16)
MAX_MAP = 1 << 24               # H * W the entry point takes: the reference's index arithmetic is fp32


def _heatmaps(a, who: str) -> torch.Tensor:
    """float32 / float16 / bfloat16 heatmaps, numpy (shared, not copied) or torch, on the host or a GPU, as a detached tensor where they are."""
    if isinstance(a, np.ndarray):
        if a.dtype not in _NP_DTYPES:
            raise TypeError(f"{who}: heatmaps must be float32, float16 or bfloat16, got {a.dtype}")
        return torch.from_numpy(np.ascontiguousarray(a))
    if isinstance(a, torch.Tensor):
        if a.dtype not in _DTYPES:
            raise TypeError(f"{who}: heatmaps must be float32, float16 or bfloat16, got {a.dtype}")
        if a.device.type not in ("cpu", "cuda"):
            raise RuntimeError(f"{who}: heatmaps on unsupported device {a.device}")
        return a.detach()
    raise TypeError(f"{who}: heatmaps must be a numpy array or a torch tensor, got {type(a).__name__}")


def check_heatmap_args(heatmaps, center, scale, boxes, aspect, who: str):
    """Everything ``heatmaps_to_keypoints`` can refuse without a device -> ``(hm, geom parts, kind, aspect)``: ``hm`` [...,17,H,W] and the one or two
    geometry tensors [...,2] / [...,4], as tensors where they are."""
    hm = _heatmaps(heatmaps, who)
    if hm.dim() < 3 or hm.shape[-3] != 17 or hm.shape[-2] < 1 or hm.shape[-1] < 1:
        raise ValueError(f"{who}: expected heatmaps [...,17,H,W] with H, W >= 1, got {tuple(hm.shape)}")
    if hm.shape[-2] * hm.shape[-1] > MAX_MAP:
        raise ValueError(f"{who}: H * W must be at most 2^24, got {hm.shape[-2]} x {hm.shape[-1]}")
    lead = tuple(hm.shape[:-3])
    if boxes is None:
        if center is None or scale is None:
            raise ValueError(f"{who}: give center and scale [...,2], or boxes [...,4] with aspect")
        if aspect is not None:
            raise ValueError(f"{who}: aspect goes with boxes, not with center / scale")
        parts = (_float32(center, who, "center"), _float32(scale, who, "scale"))
        for name, t in zip(("center", "scale"), parts):
            if tuple(t.shape) != lead + (2,):
                raise ValueError(f"{who}: expected {name} {list(lead) + [2]} for heatmaps {tuple(hm.shape)}, got {tuple(t.shape)}")
        return hm, parts, _lib.GEOM_CENTER_SCALE, 1.0
    if center is not None or scale is not None:
        raise ValueError(f"{who}: give center and scale, or boxes and aspect, not both")
    if aspect is None:
        raise ValueError(f"{who}: boxes need aspect (the demo's is frame_height / frame_width)")
    aspect = float(aspect)
    if not aspect > 0.0 or not np.isfinite(aspect):
        raise ValueError(f"{who}: aspect must be a positive finite number, got {aspect!r}")
    parts = (_float32(boxes, who, "boxes"),)
    if tuple(parts[0].shape) != lead + (4,):
        raise ValueError(f"{who}: expected boxes {list(lead) + [4]} for heatmaps {tuple(hm.shape)}, got {tuple(parts[0].shape)}")
    return hm, parts, _lib.GEOM_BOX, aspect


def heatmaps_to_keypoints(heatmaps, center=None, scale=None, *, boxes=None, aspect=None, refine: bool = True, layout: str = "coco",
                          device=None) -> torch.Tensor:
    """Pose-network heatmaps -> keypoints in image pixels: ``heatmaps`` [...,17,H,W], float32, float16 or bfloat16 (the 16-bit types are widened on load,
    exactly), a torch tensor on the GPU -- the normal case: read in place when contiguous (a strided view is packed first), never modified -- or numpy /
    torch on the host, which is uploaded.  Returns CUDA fp32 [...,17,3]: image x, image y, score (the map's maximum; a map that holds a NaN scores NaN).

    Where each person's crop sits in the image: ``center`` and ``scale`` [...,2], the pair the crop was made with (only ``scale[..., 0]`` enters, as in
    the reference); or ``boxes`` [...,4] = x1, y1, x2, y2 with ``aspect``, from which center and scale are derived as ``box_to_center_scale`` does
    (demo/lib/hrnet/lib/utils/utilitys.py:102-135) with ``aspect`` as its ``model_image_width / model_image_height``.  The demo passes
    ``frame_height / frame_width`` there (utilitys.py:151); nothing is assumed here, pass what the crops were made with.  float32, host or device.

    ``refine``: the quarter-pixel step towards the higher neighbour (the demo's ``TEST.POST_PROCESS``).  ``layout``: "coco", the network's joint order,
    or "h36m", ``coco_to_h36m`` of that result bit for bit (one more launch).  ``device``: where host input goes (default: the current GPU); GPU input
    stays where it is.  There is no host path: without a GPU the call raises ``RuntimeError``.  Exception types as ``coco_to_h36m``; every refusal comes
    before any launch."""
    who = "heatmaps_to_keypoints"
    h36m = not check_layout(layout, who)
    hm, parts, kind, aspect = check_heatmap_args(heatmaps, center, scale, boxes, aspect, who)
    on_gpu = [t.device for t in (hm,) + parts if t.is_cuda]
    if device is not None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{who}: device must be a GPU, got {dev}; kasportsformer_amd has no CPU path")
    elif on_gpu:
        dev = on_gpu[0]
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        raise RuntimeError(f"{who}: no GPU available; kasportsformer_amd has no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if any(d != dev for d in on_gpu):
        raise RuntimeError(f"{who}: input on {[str(d) for d in on_gpu]}, asked for {dev}")
    return decode(hm.to(dev), tuple(t.to(dev) for t in parts), kind, aspect, refine, h36m)


def decode(hm: torch.Tensor, parts, kind: int, aspect: float, refine: bool, h36m: bool) -> torch.Tensor:
    """``kasf_heatmap_keypoints`` on checked CUDA tensors of one device (what ``heatmaps_to_keypoints`` and ``StreamLifter.push_heatmaps`` end in)."""
    lead, (H, W) = tuple(hm.shape[:-3]), hm.shape[-2:]
    hm = hm.contiguous()                                         # the same tensor when it already is
    geom = (torch.cat(parts, dim=-1) if len(parts) == 2 else parts[0]).contiguous()
    out = torch.empty(lead + (17, 3), dtype=torch.float32, device=hm.device)
    n = out.numel() // 51
    if n:
        scratch = torch.empty_like(out) if h36m else None
        with torch.cuda.device(hm.device):
            _lib.check(_lib.load().kasf_heatmap_keypoints(hm.data_ptr(), _DTYPES[hm.dtype], n, int(H), int(W), geom.data_ptr(), kind, aspect,
                                                          int(bool(refine)), _lib.LAYOUT_H36M if h36m else _lib.LAYOUT_COCO, out.data_ptr(),
                                                          scratch.data_ptr() if h36m else None, _stream()))
    return out
