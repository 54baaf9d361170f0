"""The step between the person detector and the pose network: person boxes cropped out of a video frame to the network's input tensor, on the GPU.

    r = crop_persons(frame, boxes)                                       # frame uint8 [Hf,Wf,3] on the GPU, boxes [P,4] = x1, y1, x2, y2 (detections_to_boxes' r.boxes[b, :n, :4])
    r = crop_persons(frames, boxes, frame_index=idx)                     # frames [F,Hf,Wf,3]: person p is cropped from frames[idx[p]]
    r = crop_persons(frame, center=c, scale=s)                           # the crop geometry given instead of boxes
    r.inputs [P,3,out_h,out_w], r.center [P,2], r.scale [P,2]
    kp = heatmaps_to_keypoints(network(r.inputs), r.center, r.scale)

``crop_persons`` is the demo's ``PreProcess`` (demo/lib/hrnet/lib/utils/utilitys.py:139-169, called at demo/lib/hrnet/gen_kpts.py:152-157): per person
``box_to_center_scale``, ``get_affine_transform``, ``cv2.warpAffine(frame, trans, size, INTER_LINEAR)``, ``ToTensor``, ``Normalize``, and the ``[:, [2, 1, 0]]``
channel swap behind it -- one launch, no host copy, the same bits from run to run.  Center and scale are the reference's bit for bit; the sampling is a
restatement of the fixed-point arithmetic of OpenCV's portable ``warpAffine`` (1/32-pixel positions, integer bilinear weights, constant-0 border) that
include/kasf.h (``kasf_crop_persons``) states rule by rule.  No OpenCV build was available to record a crop from: equality with a particular cv2 build
is NOT verified.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _args, _lib

MAX_SIDE = _args.MAX_SIDE       # Hf, Wf, out_w, out_h the entry point takes
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class CropResult(NamedTuple):
    inputs: torch.Tensor       # CUDA [P, 3, out_h, out_w] of ``dtype``: what the pose network takes
    center: torch.Tensor       # CUDA fp32 [P, 2]: given, or box_to_center_scale of the box
    scale: torch.Tensor        # CUDA fp32 [P, 2]: with ``center``, what heatmaps_to_keypoints takes for the heatmaps of these crops


def _triple(value, who: str, name: str, nonzero: bool) -> np.ndarray:
    try:
        v = np.asarray(value.detach().cpu() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError(f"{who}: {name} must be three numbers, got {type(value).__name__}") from None
    if v.shape != (3,) or not np.all(np.isfinite(v)):
        raise ValueError(f"{who}: {name} must be three finite numbers, got {value!r}")
    v = v.astype(np.float32)
    if nonzero and (not np.all(np.isfinite(v)) or np.any(v == 0)):
        raise ValueError(f"{who}: every {name} must be finite and not 0 as float32, got {value!r}")
    return v


def check_crop_args(frame, boxes, center, scale, size, aspect, mean, std, dtype, frame_index, who: str):
    """Everything ``crop_persons`` can refuse without a device -> ``(frames, geom parts, kind, aspect, (out_w, out_h), mean_std [6] float32, frame_index or None)``."""
    fr = _args.frames(frame, who)
    Hf, Wf = int(fr.shape[-3]), int(fr.shape[-2])
    if boxes is None:
        if center is None or scale is None:
            raise ValueError(f"{who}: give boxes [P,4], or center and scale [P,2]")
        if aspect is not None:
            raise ValueError(f"{who}: aspect goes with boxes, not with center / scale")
        parts = (_args.as_tensor(center, who, "center", _args.FLOAT32), _args.as_tensor(scale, who, "scale", _args.FLOAT32))
        for name, t in zip(("center", "scale"), parts):
            if t.dim() != 2 or t.shape[1] != 2 or t.shape[0] != parts[0].shape[0]:
                raise ValueError(f"{who}: expected center and scale [P,2], got {name} {tuple(t.shape)}")
        kind, aspect = _lib.GEOM_CENTER_SCALE, 1.0
    else:
        if center is not None or scale is not None:
            raise ValueError(f"{who}: give boxes, or center and scale, not both")
        parts = (_args.as_tensor(boxes, who, "boxes", _args.FLOAT32),)
        if parts[0].dim() != 2 or parts[0].shape[1] != 4:
            raise ValueError(f"{who}: expected boxes [P,4] = x1, y1, x2, y2, got {tuple(parts[0].shape)}")
        aspect = Hf / Wf if aspect is None else float(aspect)        # the demo's: image.shape[0], image.shape[1] as model width, height (utilitys.py:151)
        if not aspect > 0.0 or not math.isfinite(aspect):
            raise ValueError(f"{who}: aspect must be a positive finite number, got {aspect!r}")
        kind = _lib.GEOM_BOX
    P = int(parts[0].shape[0])
    try:
        out_w, out_h = (int(v) for v in size)
    except (TypeError, ValueError):
        raise TypeError(f"{who}: size must be (width, height), got {size!r}") from None
    if not (1 <= out_w <= MAX_SIDE and 1 <= out_h <= MAX_SIDE):
        raise ValueError(f"{who}: size = (width, height) must be in [1, {MAX_SIDE}], got {size!r}")
    if dtype not in _args.DTYPES:
        raise TypeError(f"{who}: dtype must be torch.float32, torch.float16 or torch.bfloat16, got {dtype!r}")
    mean_std = np.concatenate((_triple(mean, who, "mean", False), _triple(std, who, "std", True)))
    if fr.dim() == 3:
        if frame_index is not None:
            raise ValueError(f"{who}: frame_index goes with frames [F,Hf,Wf,3], got one frame {tuple(fr.shape)}")
        fi = None
    else:
        if frame_index is None:
            raise ValueError(f"{who}: frames [F,Hf,Wf,3] need frame_index [P]")
        if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:                      # taken as it is: checking it would synchronise
            if frame_index.dtype not in (torch.int32, torch.int64):
                raise TypeError(f"{who}: frame_index must be int32 or int64, got {frame_index.dtype}")
            fi = frame_index.detach().to(torch.int32)
        else:
            v = np.asarray(frame_index.detach() if isinstance(frame_index, torch.Tensor) else frame_index)
            if v.dtype.kind not in "iu":
                raise TypeError(f"{who}: frame_index must be integers, got {v.dtype}")
            if v.ndim == 1 and v.size and (v.min() < 0 or v.max() >= fr.shape[0]):
                raise ValueError(f"{who}: frame_index must be in [0, {fr.shape[0]}), got {v.min()} .. {v.max()}")
            fi = torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32))
        if tuple(fi.shape) != (P,):
            raise ValueError(f"{who}: expected frame_index [{P}], got {tuple(fi.shape)}")
    return fr, parts, kind, aspect, (out_w, out_h), mean_std, fi


def crop_persons(frame, boxes=None, *, center=None, scale=None, size=(288, 384), aspect=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, swap_rb: bool = True,
                 dtype=torch.float32, frame_index=None, device=None) -> CropResult:
    """Person boxes -> the pose network's input: ``frame`` uint8 [Hf,Wf,3] as the decoder wrote it (the demo's is BGR), or [F,Hf,Wf,3] with ``frame_index``
    [P] naming each person's frame; a torch tensor on the GPU -- the normal case: read in place, also through a strided view with padded rows (a decoder's
    pitch) as long as the innermost two dimensions are contiguous (any other view is packed first), never modified -- or numpy / torch on the host, which
    is uploaded.  ``boxes`` [P,4] = x1, y1, x2, y2 float32, from which center and scale are derived as ``box_to_center_scale`` does with ``aspect`` as its
    ``model_image_width / model_image_height`` (default: ``Hf / Wf``, what the demo passes at utilitys.py:151); or ``center`` and ``scale`` [P,2].

    ``size``: the crop's (width, height), the reference's ``MODEL.IMAGE_SIZE``.  ``mean`` / ``std``: three numbers each, applied to the FRAME's channels by
    position; with ``swap_rb`` output plane k then holds frame channel 2 - k.  That is the demo as it is: it normalises its BGR frame with the RGB constants
    and swaps afterwards, so the red plane ends up normalised with 0.406 / 0.225.  ``dtype``: torch.float32, or float16 / bfloat16 = the round-to-nearest-even
    of the fp32 result.  ``device``: where host input goes (default: the current GPU); GPU input stays where it is.

    Returns ``CropResult(inputs [P,3,out_h,out_w], center [P,2], scale [P,2])`` on the GPU; ``heatmaps_to_keypoints(hm, r.center, r.scale)`` maps the
    network's heatmaps of ``r.inputs`` back to frame pixels.  A box that is NaN, or whose geometry is not finite, gives an all-border crop (the normalised
    value of 0), as does a ``frame_index`` entry of a GPU tensor that is out of range (a host ``frame_index`` is checked).  Sampling: include/kasf.h,
    ``kasf_crop_persons``; not verified against a cv2 build.  The detector's own letterbox and the SORT tracker are not part of this.  There is no host
    path: without a GPU the call raises ``RuntimeError``.  Exception types as ``heatmaps_to_keypoints``; every refusal comes before any launch."""
    who = "crop_persons"
    fr, parts, kind, aspect, (out_w, out_h), mean_std, fi = check_crop_args(frame, boxes, center, scale, size, aspect, mean, std, dtype, frame_index, who)
    dev = _args.resolve_device((fr,) + parts + (fi,), device, who)
    return crop(fr.to(dev), tuple(t.to(dev) for t in parts), kind, aspect, out_w, out_h, mean_std, bool(swap_rb), dtype, None if fi is None else fi.to(dev))


def crop(fr: torch.Tensor, parts, kind: int, aspect: float, out_w: int, out_h: int, mean_std: np.ndarray, swap_rb: bool, dtype, fi) -> CropResult:
    """``kasf_crop_persons`` on checked CUDA tensors of one device."""
    Hf, Wf = int(fr.shape[-3]), int(fr.shape[-2])
    if fr.stride(-1) != 1 or fr.stride(-2) != 3 or fr.stride(-3) < 3 * Wf:
        fr = fr.contiguous()                                     # only a view whose pixels are not interleaved bytes is packed
    n_frames, frame_stride = (int(fr.shape[0]), int(fr.stride(0))) if fr.dim() == 4 else (1, 0)
    geom = (torch.cat(parts, dim=-1) if len(parts) == 2 else parts[0]).contiguous()
    P = int(geom.shape[0])
    out = torch.empty((P, 3, out_h, out_w), dtype=dtype, device=fr.device)
    cs = torch.empty((P, 4), dtype=torch.float32, device=fr.device)
    if P:
        mean_std = np.ascontiguousarray(mean_std, dtype=np.float32)
        with torch.cuda.device(fr.device):
            _lib.check(_lib.load().kasf_crop_persons(fr.data_ptr(), n_frames, Hf, Wf, int(fr.stride(-3)), frame_stride, None if fi is None else fi.data_ptr(),
                                                     geom.data_ptr(), kind, float(aspect), P, out.data_ptr(), _args.DTYPES[dtype], out_w, out_h,
                                                     mean_std.ctypes.data_as(C.POINTER(C.c_float)), int(swap_rb), cs.data_ptr(), _args.stream()))
    return CropResult(out, cs[:, :2], cs[:, 2:])
