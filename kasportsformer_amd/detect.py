"""The step in front of the pose network: a YOLOv3 person detector's output decoded to person boxes on the GPU it was computed on.

    r = detections_to_boxes(prediction, width, height, inp_dim=416)      # prediction [B,N,5+C]: what the reference's Darknet.forward returns
    r = yolo_heads_to_boxes(heads, width, height, inp_dim=416)           # heads: the raw [B,A*(5+C),G,G] tensors in front of the detection layers
    r.boxes [B,max_boxes,6], r.count [B], r.candidates [B], r.index [B,max_boxes]
    kp = heatmaps_to_keypoints(hm, boxes=r.boxes[0, :n, :4], aspect=frame_h / frame_w)

Both are ``yolo_human_det`` behind the network (demo/lib/yolov3/human_detector.py:116-168): ``predict_transform`` (demo/lib/yolov3/util.py:34-81; the heads
form only), ``write_results`` with ``det_hm`` (util.py:107-225: objectness threshold, class arg-max, persons only, sort, greedy NMS with ``bbox_iou``,
demo/lib/yolov3/bbox.py:51-78) and the un-letterbox and clamp (human_detector.py:144-153) -- two launches, no host synchronisation, the same bits from
run to run.  In the prediction form every operation is a single fp32 operation in the reference's order, and the result is the reference's bit for bit;
in the heads form the device's ``exp`` stands in for the host's.  include/kasf.h (``kasf_detect_boxes``) states every rule.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _args, _lib

# the nine (width, height) anchor pairs of the public YOLOv3 configuration, in pixels of the network input, smallest first
YOLOV3_ANCHORS = ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
YOLOV3_MASKS = ((6, 7, 8), (3, 4, 5), (0, 1, 2))     # anchors of the stride-32, -16 and -8 heads, the order in which the reference concatenates them
MAX_CANDIDATES = _lib.DETECT_MAX_CANDIDATES             # the largest ``max_candidates``: sort and NMS run in one compute unit's LDS
MAX_BATCH, MAX_PER_IMAGE = 65535, 1 << 24


class DetectResult(NamedTuple):
    boxes: torch.Tensor        # CUDA fp32 [B, max_boxes, 6]: x1, y1, x2, y2 in frame pixels (clamped to the frame), objectness, class score; rows past count are 0
    count: torch.Tensor        # CUDA int32 [B]: rows written for each image
    candidates: torch.Tensor   # CUDA int32 [B]: candidates that passed the threshold and the class filter, before NMS and before any cap
    index: torch.Tensor        # CUDA int32 [B, max_boxes]: candidate index of each row (position in the reference's concatenated prediction), -1 past count


def _frame(value, B: int, who: str, name: str):
    """``width`` / ``height``: one number, or one per image as a [B] array / tensor.  A GPU tensor is taken as it is (checking it would synchronise)."""
    if isinstance(value, torch.Tensor) and value.is_cuda:
        if tuple(value.shape) != (B,):
            raise ValueError(f"{who}: {name} must be one value or one per image ({B}), got shape {tuple(value.shape)}")
        return value.detach().to(torch.float32)
    try:
        v = np.asarray(value.detach() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError(f"{who}: {name} must be a number or a [B] array / tensor, got {type(value).__name__}") from None
    if v.ndim == 0:
        v = np.full(B, v)
    elif v.shape != (B,):
        raise ValueError(f"{who}: {name} must be one value or one per image ({B}), got shape {v.shape}")
    v = v.astype(np.float32)
    if not np.all(v > 0) or not np.all(np.isfinite(v)):
        raise ValueError(f"{who}: width and height must be positive and finite")
    return torch.from_numpy(v)


def check_detect_args(src, form: int, width, height, inp_dim, confidence, nms, class_id, max_boxes, max_candidates, who: str,
                      anchors=None, masks=None, num_classes=None):
    """Everything the two calls can refuse without a device -> ``(tensors, B, grids, A, C, anchors [n_src*A*2] float32 or None, width, height)``."""
    if form == _lib.DETECT_PREDICTION:
        t = _args.as_tensor(src, who, "prediction", _args.DTYPES)
        if t.dim() != 3 or t.shape[2] < 6 or t.shape[1] < 1:
            raise ValueError(f"{who}: expected prediction [B,N,5+C] with N >= 1 and C >= 1, got {tuple(t.shape)}")
        tensors, B, grids, A, Cn, anc = [t], int(t.shape[0]), [int(t.shape[1])], 1, int(t.shape[2]) - 5, None
        n_per_image = grids[0]
    else:
        if isinstance(src, (np.ndarray, torch.Tensor)) or not hasattr(src, "__len__"):
            raise TypeError(f"{who}: heads must be a sequence of tensors, one per detection layer")
        if not 1 <= len(src) <= 4:
            raise ValueError(f"{who}: 1 to 4 heads, got {len(src)}")
        tensors = [_args.as_tensor(h, who, f"heads[{k}]", _args.DTYPES) for k, h in enumerate(src)]
        if len({t.dtype for t in tensors}) != 1:
            raise TypeError(f"{who}: all heads must have one dtype, got {[str(t.dtype) for t in tensors]}")
        Cn = int(num_classes)
        if Cn < 1:
            raise ValueError(f"{who}: num_classes must be >= 1, got {num_classes}")
        if masks is None or len(masks) != len(tensors):
            raise ValueError(f"{who}: masks must hold one tuple of anchor numbers per head ({len(tensors)})")
        A = len(masks[0])
        if not 1 <= A <= 8 or any(len(m) != A for m in masks):
            raise ValueError(f"{who}: every head takes the same number of anchors, 1 to 8; got masks {masks!r}")
        table = np.asarray(anchors, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 2 or not np.all(np.isfinite(table)) or not np.all(table > 0):
            raise ValueError(f"{who}: anchors must be positive (width, height) pairs")
        flat = [int(i) for m in masks for i in m]
        if any(i < 0 or i >= len(table) for i in flat):
            raise ValueError(f"{who}: masks name anchors outside 0..{len(table) - 1}")
        anc = np.ascontiguousarray(table[flat].reshape(-1), dtype=np.float32)
        B, grids = int(tensors[0].shape[0]) if tensors[0].dim() == 4 else -1, []
        for k, t in enumerate(tensors):
            if t.dim() != 4 or t.shape[0] != B or t.shape[1] != A * (5 + Cn) or t.shape[2] != t.shape[3] or t.shape[2] < 1:
                raise ValueError(f"{who}: expected heads[{k}] [B,{A * (5 + Cn)},G,G] (A = {A}, num_classes = {Cn}), got {tuple(t.shape)}")
            grids.append(int(t.shape[2]))
        n_per_image = sum(g * g * A for g in grids)
    inp_dim = int(inp_dim)
    if inp_dim < 1:
        raise ValueError(f"{who}: inp_dim must be positive, got {inp_dim}")
    if form == _lib.DETECT_HEADS and any(g > 4096 or inp_dim % g for g in grids):
        raise ValueError(f"{who}: every head's grid must divide inp_dim = {inp_dim}, got grids {grids}")
    if B > MAX_BATCH or n_per_image > MAX_PER_IMAGE:
        raise ValueError(f"{who}: at most {MAX_BATCH} images of at most 2^24 candidates each, got {B} x {n_per_image}")
    confidence, nms = float(confidence), float(nms)
    if not (math.isfinite(confidence) and math.isfinite(nms)):
        raise ValueError(f"{who}: confidence and nms must be finite, got {confidence!r}, {nms!r}")
    class_id, max_boxes, max_candidates = int(class_id), int(max_boxes), int(max_candidates)
    if not 0 <= class_id < Cn:
        raise ValueError(f"{who}: class_id must be in [0, {Cn}), got {class_id}")
    if not 1 <= max_candidates <= MAX_CANDIDATES:
        raise ValueError(f"{who}: max_candidates must be in [1, {MAX_CANDIDATES}], got {max_candidates}")
    if not 1 <= max_boxes <= max_candidates:
        raise ValueError(f"{who}: max_boxes must be in [1, max_candidates = {max_candidates}], got {max_boxes}")
    return tensors, B, grids, A, Cn, anc, _frame(width, B, who, "width"), _frame(height, B, who, "height")


def _run(src, form, width, height, inp_dim, confidence, nms, class_id, max_boxes, max_candidates, device, who, **heads_kw) -> DetectResult:
    tensors, B, grids, A, Cn, anc, w, h = check_detect_args(src, form, width, height, inp_dim, confidence, nms, class_id, max_boxes, max_candidates, who,
                                                            **heads_kw)
    dev = _args.resolve_device(tensors + [w, h], device, who)
    max_boxes, max_candidates = int(max_boxes), int(max_candidates)
    tensors = [t.to(dev).contiguous() for t in tensors]          # the same tensor when it is on the device and contiguous
    frame_wh = torch.stack((w.to(dev), h.to(dev)), dim=1).contiguous()
    boxes = torch.empty((B, max_boxes, 6), dtype=torch.float32, device=dev)
    index = torch.empty((B, max_boxes), dtype=torch.int32, device=dev)
    count = torch.empty((B, 2), dtype=torch.int32, device=dev)
    if B:
        lib = _lib.load()
        n_per_image = grids[0] if form == _lib.DETECT_PREDICTION else sum(g * g * A for g in grids)
        nbytes = lib.kasf_detect_workspace_bytes(B, n_per_image, max_candidates)
        if nbytes < 0:
            _lib.check(2)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        grid = (C.c_int32 * len(grids))(*grids)
        anchors = anc.ctypes.data_as(C.POINTER(C.c_float)) if anc is not None else None
        with torch.cuda.device(dev):
            _lib.check(lib.kasf_detect_boxes(ptrs, len(tensors), form, _args.DTYPES[tensors[0].dtype], B, grid, A, Cn, anchors, int(inp_dim), frame_wh.data_ptr(),
                                             float(confidence), float(nms), int(class_id), max_candidates, max_boxes, boxes.data_ptr(), index.data_ptr(),
                                             count.data_ptr(), ws.data_ptr(), nbytes, _args.stream()))
    return DetectResult(boxes, count[:, 0], count[:, 1], index)


_COMMON = """``width`` / ``height``: the frame's size in pixels, one number for all images or one per image as a [B] array / tensor (a GPU tensor is taken as it
    is).  ``confidence``: the objectness a candidate must exceed; 0.70 is ``yolo_human_det``'s default, the demo passes 0.30 (demo/lib/hrnet/gen_kpts.py:62,123).
    ``nms``: a box survives a better one iff their IoU is below it.  ``class_id``: the class kept (0 = person).  ``max_boxes``: rows of the result.
    ``max_candidates``: how many of the best candidates enter NMS, at most 4096; ``r.candidates`` shows whether that cap bit, and a capped result is a
    prefix of the uncapped one.  ``device``: where host input goes (default: the current GPU); GPU input stays where it is.

    Input is float32, float16 or bfloat16 (the 16-bit types are widened on load, exactly), a torch tensor on the GPU -- read in place when contiguous (a
    strided view is packed first), never modified -- or numpy / torch on the host, which is uploaded.  Returns ``DetectResult(boxes, count, candidates,
    index)``; ``r.boxes[b, :n, :4]`` is what ``heatmaps_to_keypoints(boxes=...)`` takes.  Nothing in the call synchronises with the host.

    Deliberately unlike the reference: images of a batch are independent (``write_results`` returns at the first image without a person; here that image
    has count 0 and the others are unaffected); equal objectness is ordered by candidate index; a candidate with a NaN objectness or a non-finite box is
    dropped; the host-side ``round(i, 2)`` and the SORT tracker are not part of this.  There is no host path: without a GPU the call raises
    ``RuntimeError``.  Exception types as ``heatmaps_to_keypoints``; every refusal comes before any launch."""


def detections_to_boxes(prediction, width, height, inp_dim: int = 416, *, confidence: float = 0.70, nms: float = 0.4, class_id: int = 0,
                        max_boxes: int = 32, max_candidates: int = 1024, device=None) -> DetectResult:
    return _run(prediction, _lib.DETECT_PREDICTION, width, height, inp_dim, confidence, nms, class_id, max_boxes, max_candidates, device,
                "detections_to_boxes")


def yolo_heads_to_boxes(heads, width, height, inp_dim: int = 416, *, anchors=YOLOV3_ANCHORS, masks=YOLOV3_MASKS, num_classes: int = 80,
                        confidence: float = 0.70, nms: float = 0.4, class_id: int = 0, max_boxes: int = 32, max_candidates: int = 1024,
                        device=None) -> DetectResult:
    return _run(heads, _lib.DETECT_HEADS, width, height, inp_dim, confidence, nms, class_id, max_boxes, max_candidates, device, "yolo_heads_to_boxes",
                anchors=anchors, masks=masks, num_classes=num_classes)


detections_to_boxes.__doc__ = """A YOLOv3 detector's decoded output -> person boxes in frame pixels: ``prediction`` [B,N,5+C] = x, y, w, h at network-input scale,
    objectness, C class scores per candidate, what the reference's ``Darknet.forward`` returns.  ``write_results`` with ``det_hm`` and the un-letterbox of
    ``yolo_human_det``; the result is the reference's bit for bit.  ``inp_dim``: the side of the square network input the frame was letterboxed into.

    """ + _COMMON
yolo_heads_to_boxes.__doc__ = """The same from the raw detection heads: ``heads`` = a sequence of [B,A*(5+C),G,G] tensors as the conv layers in front of the detection
    layers write them, stride 32 first (the order in which the reference concatenates them); ``predict_transform`` is applied on the fly, to passing
    candidates only, and no transposed [N,5+C] copy is made.  ``anchors``: (width, height) pairs in network-input pixels; ``masks``: one tuple of anchor
    numbers per head, in the order of ``heads``; ``num_classes``: C.  ``inp_dim`` must be a multiple of every G.  The class arg-max is taken on the logits
    (one sigmoid for the winner): the reference's differs only where two class scores round to the same fp32 sigmoid.

    """ + _COMMON
