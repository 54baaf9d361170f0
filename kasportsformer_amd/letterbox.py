"""The step in front of the person detector: video frames letterboxed to the YOLOv3 network's input tensor, on the GPU.

    r = letterbox_frames(frame, inp_dim=416)                  # frame uint8 [Hf,Wf,3] or [F,Hf,Wf,3] on the GPU; inp_dim = one int or (width, height)
    r.inputs [F,3,h,w] ([1,3,h,w] for one frame), r.width, r.height (the frame's), r.size = (new_w, new_h), r.offset = (pad_x, pad_y)
    d = yolo_heads_to_boxes(detector(r.inputs), r.width, r.height, inp_dim=416, confidence=0.30)

``letterbox_frames`` is the demo's ``prep_image`` (demo/lib/yolov3/preprocess.py:9-38, called at demo/lib/yolov3/human_detector.py:131): ``letterbox_image`` =
``cv2.resize(frame, (new_w, new_h), INTER_CUBIC)`` placed on a canvas of 128, the ``[:, :, ::-1]`` channel reversal, the transpose to planes and
``float().div(255.0)`` -- one launch that writes the padding too, no host copy, the same bits from run to run.  ``new_w``, ``new_h`` and the placement are the
reference's bit for bit; the resampling is a restatement of the fixed-point arithmetic of OpenCV's portable 8-bit ``resize(INTER_CUBIC)`` (11-bit
coefficients, integer sums, a 22-bit rounding shift, replicated edge) that include/kasf.h (``kasf_letterbox_frames``) states rule by rule, within 1.25 grey
levels of exact cubic convolution on every pixel.  No OpenCV build was available to record an image from, and cv2's SIMD paths may round differently:
equality with a particular cv2 build is NOT verified.
"""
from __future__ import annotations

import ctypes as C
import operator
from typing import NamedTuple, Tuple

import torch

from . import _args, _lib

MAX_SIDE = _lib.LETTERBOX_MAX_SIDE      # out_w, out_h the entry point takes


class LetterboxResult(NamedTuple):
    inputs: torch.Tensor            # CUDA [F, 3, h, w] of ``dtype``: what the detector network takes
    width: int                      # the frame's width and height: what yolo_heads_to_boxes / detections_to_boxes take to undo the letterbox
    height: int
    size: Tuple[int, int]           # (new_w, new_h) of the resized image inside the input
    offset: Tuple[int, int]         # (pad_x, pad_y): its top-left corner; host integers from the plan, nothing is read back


def letterbox_plan(width: int, height: int, out_w: int, out_h: int, who: str = "letterbox_plan"):
    """``kasf_letterbox_plan`` (host arithmetic only, no device): ``((new_w, new_h), (pad_x, pad_y))`` of the reference's ``letterbox_image`` for a frame of
    ``width`` x ``height`` in an input of ``out_w`` x ``out_h``; ``ValueError`` where the entry point refuses (a size out of range, or ``new_w`` or ``new_h`` < 1)."""
    v = [C.c_int32() for _ in range(4)]
    if _lib.load().kasf_letterbox_plan(int(width), int(height), int(out_w), int(out_h), *(C.byref(x) for x in v)) != 0:
        raise ValueError(f"{who}: a {width} x {height} frame has no letterbox in {out_w} x {out_h}: frame sides must be in [1, 32767], input sides in "
                         f"[1, {MAX_SIDE}], and the resized image must keep at least one pixel per side")
    return (v[0].value, v[1].value), (v[2].value, v[3].value)


def check_letterbox_args(frame, inp_dim, pad, dtype, who: str):
    """Everything ``letterbox_frames`` can refuse without a device -> ``(frames, (out_w, out_h), pad, (new_w, new_h), (pad_x, pad_y))``."""
    fr = _args.frames(frame, who)
    if isinstance(inp_dim, bool):
        raise TypeError(f"{who}: inp_dim must be an int or (width, height), got {inp_dim!r}")
    try:
        out_w = out_h = operator.index(inp_dim)
    except TypeError:
        try:
            out_w, out_h = (operator.index(v) for v in inp_dim)
        except (TypeError, ValueError):
            raise TypeError(f"{who}: inp_dim must be an int or (width, height), got {inp_dim!r}") from None
    if not (1 <= out_w <= MAX_SIDE and 1 <= out_h <= MAX_SIDE):
        raise ValueError(f"{who}: inp_dim = (width, height) must be in [1, {MAX_SIDE}], got {inp_dim!r}")
    pad = _args.index_in(pad, who, "pad", 0, 255, any_index=True)
    if dtype not in _args.DTYPES:
        raise TypeError(f"{who}: dtype must be torch.float32, torch.float16 or torch.bfloat16, got {dtype!r}")
    size, offset = letterbox_plan(int(fr.shape[-2]), int(fr.shape[-3]), out_w, out_h, who)
    return fr, (out_w, out_h), pad, size, offset


def letterbox_frames(frame, inp_dim=416, *, pad: int = 128, swap_rb: bool = True, dtype=torch.float32, device=None) -> LetterboxResult:
    """Video frames -> the detector network's input: ``frame`` uint8 [Hf,Wf,3] as the decoder wrote it (the demo's is BGR), or [F,Hf,Wf,3], all of one size; a
    torch tensor on the GPU -- the normal case: read in place, also through a strided view with padded rows (a decoder's pitch) as long as the innermost two
    dimensions are contiguous (any other view is packed first), never modified -- or numpy / torch on the host, which is uploaded.  These are ``crop_persons``'
    rules for its frames, unchanged.

    ``inp_dim``: the network's input side, or (width, height); at most 4096 per side.  ``pad``: the canvas value, 0..255 (the reference: 128).  ``swap_rb``:
    output plane k holds frame channel 2 - k, the reference's ``[:, :, ::-1]``.  ``dtype``: torch.float32, or float16 / bfloat16 = the round-to-nearest-even of
    the fp32 result.  ``device``: where host input goes (default: the current GPU); GPU input stays where it is.

    Returns ``LetterboxResult(inputs [F,3,h,w], width, height, size, offset)``: ``inputs`` on the GPU ([1,3,h,w] for one frame, as ``prep_image``'s
    ``unsqueeze(0)``), every element written by the one launch; the rest are host integers (the frame's width and height, which ``yolo_heads_to_boxes`` takes
    to undo the letterbox; ``(new_w, new_h)`` and ``(pad_x, pad_y)`` of the resized image), computed on the host: nothing is read back.  A frame so
    elongated that ``new_w`` or ``new_h`` would be 0 -- the reference's ``cv2.resize`` raises there -- is a ``ValueError``.  Resampling: include/kasf.h,
    ``kasf_letterbox_frames``; within 1.25 grey levels of exact cubic convolution, not verified against a cv2 build.  There is no host path: without a GPU the
    call raises ``RuntimeError``.  Exception types as ``crop_persons``; every refusal comes before any launch."""
    who = "letterbox_frames"
    fr, (out_w, out_h), pad, size, offset = check_letterbox_args(frame, inp_dim, pad, dtype, who)
    dev = _args.resolve_device((fr,), device, who)
    inputs = letterbox(fr.to(dev), out_w, out_h, pad, bool(swap_rb), dtype)
    return LetterboxResult(inputs, int(fr.shape[-2]), int(fr.shape[-3]), size, offset)


def letterbox(fr: torch.Tensor, out_w: int, out_h: int, pad: int, swap_rb: bool, dtype) -> torch.Tensor:
    """``kasf_letterbox_frames`` on checked CUDA frames."""
    Hf, Wf = int(fr.shape[-3]), int(fr.shape[-2])
    if fr.stride(-1) != 1 or fr.stride(-2) != 3 or fr.stride(-3) < 3 * Wf or (fr.dim() == 4 and fr.shape[0] > 1 and fr.stride(0) < Hf * fr.stride(-3)):
        fr = fr.contiguous()                                     # only a view whose pixels are not interleaved bytes, or whose frames overlap, is packed
    n_frames, frame_stride = (int(fr.shape[0]), int(fr.stride(0))) if fr.dim() == 4 else (1, 0)
    if n_frames == 1:
        frame_stride = 0
    out = torch.empty((n_frames, 3, out_h, out_w), dtype=dtype, device=fr.device)
    with torch.cuda.device(fr.device):
        _lib.check(_lib.load().kasf_letterbox_frames(fr.data_ptr(), n_frames, Hf, Wf, int(fr.stride(-3)), frame_stride, out.data_ptr(), _args.DTYPES[dtype], out_w,
                                                     out_h, pad, int(swap_rb), _args.stream()))
    return out
