"""The step in front of ``coco_to_h36m``: a top-down pose network's heatmaps decoded to keypoints on the GPU they were computed on.

    kp = heatmaps_to_keypoints(hm, center, scale)                         # hm [...,17,H,W] on the GPU -> CUDA fp32 [...,17,3] COCO-17 image x, y, score
    kp = heatmaps_to_keypoints(hm, boxes=boxes, aspect=frame_h / frame_w) # the detector's boxes instead of the crop's center / scale
    kp = heatmaps_to_keypoints(hm, center, scale, layout="h36m")          # ... and through coco_to_h36m: what lift_track / lift_tracks take
    poses = lifter.push_heatmaps(hm, center, scale)                       # StreamLifter: decode, then push
    kp = heatmaps_to_keypoints(hm, center, scale, flipped=hm_of_mirrored_crops)   # the flip test: mirror back, swap left / right, shift, average, decode: one launch
    kp = heatmaps_to_keypoints(hm, center, scale, decode="dark_udp")      # ViTPose / *_udp checkpoints: DARK-UDP sub-pixel step, W - 1 / H - 1 affine; "dark": *_dark

``heatmaps_to_keypoints`` is ``get_final_preds`` (demo/lib/hrnet/lib/utils/inference.py:21-82: argmax per joint map, the quarter-pixel ``POST_PROCESS``
step, ``transform_preds`` back to image pixels), which the demo runs on the host on a copy of HRNet's output (demo/lib/hrnet/gen_kpts.py:158-161); HRNet,
ViTPose and SimpleBaseline all end in it.  Positions, scores and refined heatmap coordinates are the reference's bit for bit; the image coordinates are the
closed form of its three-point affine evaluated in fp64 and rounded once, within 1 fp32 ulp of what the reference's ``cv2.getAffineTransform`` solve
gives (include/kasf.h, ``kasf_heatmap_keypoints``, states every rule).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _args, _lib
from .pose import check_layout

MAX_MAP = 1 << 24               # H * W the entry point takes: the reference's index arithmetic is fp32
COCO_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))      # flip_back's matched_parts for COCO-17; joint 0 is its own partner


class FlipDecode(NamedTuple):
    """``heatmaps_to_keypoints(..., flipped=..., merged=...)``: the keypoints [...,17,3] and the fp32 merged maps [...,17,H,W] they were decoded from."""
    keypoints: torch.Tensor
    merged: torch.Tensor


def check_heatmap_args(heatmaps, center, scale, boxes, aspect, who: str):
    """Everything ``heatmaps_to_keypoints`` can refuse without a device -> ``(hm, geom parts, kind, aspect)``: ``hm`` [...,17,H,W] and the one or two
    geometry tensors [...,2] / [...,4], as tensors where they are."""
    hm = _args.as_tensor(heatmaps, who, "heatmaps", _args.DTYPES)
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
        parts = (_args.as_tensor(center, who, "center", _args.FLOAT32), _args.as_tensor(scale, who, "scale", _args.FLOAT32))
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
    parts = (_args.as_tensor(boxes, who, "boxes", _args.FLOAT32),)
    if tuple(parts[0].shape) != lead + (4,):
        raise ValueError(f"{who}: expected boxes {list(lead) + [4]} for heatmaps {tuple(hm.shape)}, got {tuple(parts[0].shape)}")
    return hm, parts, _lib.GEOM_BOX, aspect


def partner_table(pairs, who: str) -> np.ndarray:
    """``pairs=`` of a flip-tested call -> int32 [17], joint j's partner (itself when unpaired): None = ``COCO_PAIRS``; otherwise a sequence of ``(a, b)``
    with distinct integers in 0..16, every joint in at most one pair -- so the table is an involution, as ``kasf_heatmap_flip_keypoints`` requires."""
    if pairs is None:
        pairs = COCO_PAIRS
    if isinstance(pairs, (str, bytes)) or not hasattr(pairs, "__iter__"):
        raise TypeError(f"{who}: pairs must be a sequence of (a, b) joint pairs, got {type(pairs).__name__}")
    table = np.arange(17, dtype=np.int32)
    for pair in pairs:
        try:
            a, b = pair
        except (TypeError, ValueError):
            raise ValueError(f"{who}: pairs must hold (a, b) joint pairs, got {pair!r}") from None
        for v in (a, b):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{who}: joint indices in pairs must be integers, got {v!r}")
            if not 0 <= v <= 16:
                raise ValueError(f"{who}: joint indices in pairs must be in [0, 16], got {v}")
        if a == b or table[a] != a or table[b] != b:
            raise ValueError(f"{who}: every joint may appear in at most one pair, and not with itself: {tuple(pair)!r}")
        table[a], table[b] = b, a
    return table


def check_flip_args(hm: torch.Tensor, flipped, shift, pairs, who: str):
    """What the flip test adds to ``check_heatmap_args``, refused without a device -> ``None`` without ``flipped`` (``shift`` / ``pairs`` must then be at
    their defaults), else ``(hmf, shift, partner)``: the flipped heatmaps as a tensor where they are, of ``hm``'s shape and dtype, and ``partner_table``."""
    if flipped is None:
        if shift is not True or pairs is not None:
            raise ValueError(f"{who}: shift and pairs go with flipped=")
        return None
    hmf = _args.as_tensor(flipped, who, "heatmaps", _args.DTYPES)
    if tuple(hmf.shape) != tuple(hm.shape) or hmf.dtype != hm.dtype:
        raise ValueError(f"{who}: flipped must have the heatmaps' shape and dtype, {tuple(hm.shape)} {hm.dtype}, got {tuple(hmf.shape)} {hmf.dtype}")
    if not isinstance(shift, (bool, np.bool_)):
        raise TypeError(f"{who}: shift must be a bool, got {shift!r}")
    return hmf, bool(shift), partner_table(pairs, who)


DECODES = {"quarter": _lib.DECODE_QUARTER, "dark": _lib.DECODE_DARK, "dark_udp": _lib.DECODE_DARK_UDP}
_FIXED_WEIGHTS = {1: (1.0,), 3: (0.25, 0.5, 0.25), 5: (0.0625, 0.25, 0.375, 0.25, 0.0625),
                  7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125)}     # OpenCV's tables for sigma <= 0


def _check_kernel(kernel, who: str) -> int:
    if isinstance(kernel, (bool, np.bool_)) or not isinstance(kernel, (int, np.integer)):
        raise TypeError(f"{who}: kernel must be an odd integer in [1, 17], got {kernel!r}")
    if not 1 <= kernel <= 17 or kernel % 2 == 0:
        raise ValueError(f"{who}: kernel must be an odd integer in [1, 17], got {kernel}")
    return int(kernel)


def _check_sigma(sigma, who: str) -> float:
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: sigma must be a positive finite number, got {sigma!r}")
    if not sigma > 0 or not np.isfinite(sigma):
        raise ValueError(f"{who}: sigma must be a positive finite number, got {sigma!r}")
    return float(sigma)


def gaussian_weights(kernel: int = 11, sigma=None) -> np.ndarray:
    """The ``kernel`` weights of the DARK decodes' separable Gaussian, float32 (include/kasf.h, ``kasf_heatmap_decode``): computed in float64 and rounded once.
    ``kernel`` odd, 1..17.  Without ``sigma`` and for 1, 3, 5, 7 taps OpenCV's fixed tables; otherwise ``sigma = ((kernel - 1) * 0.5 - 1) * 0.3 + 0.8`` when none
    is given (``cv2.GaussianBlur(..., (k, k), 0)``, what mmpose calls), ``w_i = exp(-(i - (kernel - 1) / 2)^2 / (2 sigma^2))`` divided by their sum."""
    who = "gaussian_weights"
    K = _check_kernel(kernel, who)
    if sigma is None and K in _FIXED_WEIGHTS:
        return np.array(_FIXED_WEIGHTS[K], dtype=np.float32)
    sigma = ((K - 1) * 0.5 - 1) * 0.3 + 0.8 if sigma is None else _check_sigma(sigma, who)
    i = np.arange(K, dtype=np.float64) - (K - 1) / 2
    w = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


def check_decode_args(hm: torch.Tensor, decode, kernel, sigma, udp, refine, who: str):
    """``decode`` / ``kernel`` / ``sigma`` / ``udp``, refused without a device -> ``None`` when all four are at their defaults (the existing entries serve the
    call, as before), else ``(mode, weights, udp)`` for ``kasf_heatmap_decode``: weights float32 [kernel] on the host, None with "quarter"."""
    if not isinstance(decode, str) or decode not in DECODES:
        raise ValueError(f"{who}: decode must be one of {', '.join(repr(k) for k in DECODES)}, got {decode!r}")
    if udp is not None and not isinstance(udp, (bool, np.bool_)):
        raise TypeError(f"{who}: udp must be None or a bool, got {udp!r}")
    mode = DECODES[decode]
    weights = None
    if mode == _lib.DECODE_QUARTER:
        if kernel is not None or sigma is not None:
            raise ValueError(f"{who}: kernel and sigma go with decode='dark' or 'dark_udp'")
    else:
        if not refine:
            raise ValueError(f"{who}: refine=False goes with decode='quarter' only: the DARK step is the refinement")
        K = 11 if kernel is None else _check_kernel(kernel, who)
        weights = gaussian_weights(K, None if sigma is None else _check_sigma(sigma, who))
    udp = mode == _lib.DECODE_DARK_UDP if udp is None else bool(udp)
    if udp and (hm.shape[-2] < 2 or hm.shape[-1] < 2):
        raise ValueError(f"{who}: udp needs maps of at least 2 x 2, got {hm.shape[-2]} x {hm.shape[-1]}")
    if mode == _lib.DECODE_QUARTER and not udp:
        return None
    if not refine:
        raise ValueError(f"{who}: refine=False is not available with udp=True")
    return mode, weights, udp


def _check_merged(merged, hm: torch.Tensor, flip, who: str):
    """``merged=`` -> None, True, or the caller's tensor: contiguous CUDA fp32 of the heatmaps' shape."""
    if merged is None or merged is False:
        return None
    if flip is None:
        raise ValueError(f"{who}: merged goes with flipped=")
    if merged is True:
        return True
    if not isinstance(merged, torch.Tensor):
        raise TypeError(f"{who}: merged must be True or a CUDA float32 tensor, got {type(merged).__name__}")
    if merged.dtype != torch.float32:
        raise TypeError(f"{who}: merged must be float32, got {merged.dtype}")
    if not merged.is_cuda:
        raise RuntimeError(f"{who}: merged must be on the GPU, got {merged.device}")
    if tuple(merged.shape) != tuple(hm.shape) or not merged.is_contiguous():
        raise ValueError(f"{who}: merged must be contiguous {tuple(hm.shape)}, got {tuple(merged.shape)} with strides {merged.stride()}")
    return merged


def _spans_overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Do the address ranges that two non-empty tensors of one device span intersect?  (No dereference: sizes and strides only.)"""
    def span(t):
        first = t.data_ptr()
        return first, first + (sum((n - 1) * abs(s) for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def heatmaps_to_keypoints(heatmaps, center=None, scale=None, *, boxes=None, aspect=None, refine: bool = True, layout: str = "coco",
                          device=None, flipped=None, shift: bool = True, pairs=None, merged=None, decode: str = "quarter", kernel=None, sigma=None, udp=None):
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
    before any launch.

    The flip test (HRNet's ``FLIP_TEST`` with ``SHIFT_HEATMAP``; one launch, ``kasf_heatmap_flip_keypoints``): ``flipped`` = the network's output for the
    mirrored crops (``inputs.flip(-1)``), of the heatmaps' shape and dtype, given as ``heatmaps`` may be.  The keypoints are then decoded from
    ``merged[..., j, y, x] = (heatmaps[..., j, y, x] + flipped[..., partner[j], y, src_x]) * 0.5`` in float32, ``src_x = min(W - x, W - 1)`` with ``shift``
    (the mirrored map moved one column right, column 0 keeping its value) and ``W - 1 - x`` without.  For 16-bit input this is deliberately not what half
    arithmetic on the tensors gives: it is the reference's float32 procedure on the exact upcasts.  ``pairs``: the left / right joint pairs ``(a, b)``
    (default ``COCO_PAIRS``; ``[]`` swaps nothing).  ``merged=True`` also returns the fp32 merged maps [...,17,H,W]; ``merged=tensor`` writes them into the
    caller's contiguous CUDA float32 tensor of that shape.  With ``merged`` the call returns ``FlipDecode(keypoints, merged)``, otherwise the keypoints alone.
    ``shift`` / ``pairs`` / ``merged`` without ``flipped`` raise ``ValueError``; without ``flipped`` the call is the plain decode, unchanged.

    Sub-pixel refinement (``kasf_heatmap_decode``, still one launch; include/kasf.h states every rule): ``decode="quarter"`` is the rule above, what HRNet's
    own checkpoints use.  ``"dark"`` is DARK (Zhang et al., CVPR 2020; mmpose's ``post_process='unbiased'``, the ``*_dark`` checkpoints), ``"dark_udp"`` the
    DARK step of UDP (Huang et al., CVPR 2020; mmpose's ``post_dark_udp``, ViTPose and the ``*_udp`` checkpoints): the map is blurred with a ``kernel``-tap
    Gaussian (odd, 1..17, default 11; ``sigma`` default OpenCV's rule for that size, see ``gaussian_weights``) and logged around the argmax only, and one
    Newton step is made from there; argmax and score still come from the raw (or merged) map.  ``udp``: map heatmap coordinates back over ``W - 1`` /
    ``H - 1`` intervals, each axis by its own scale, for crops made the UDP way; ``None`` means ``decode == "dark_udp"``, and ``udp=True`` with ``"quarter"``
    is allowed.  Everything composes with ``flipped`` / ``merged``, ``boxes`` and ``layout``.  ``kernel`` / ``sigma`` with ``"quarter"``, ``refine=False`` with a
    DARK mode or with ``udp=True``, and ``udp=True`` on a map with a side of 1 raise ``ValueError``.  With all four at their defaults the call launches exactly
    what it launched before.  The rules restate mmpose's and OpenCV's published arithmetic; equality with a particular mmpose / cv2 build is not verified."""
    who = "heatmaps_to_keypoints"
    h36m = not check_layout(layout, who)
    hm, parts, kind, aspect = check_heatmap_args(heatmaps, center, scale, boxes, aspect, who)
    flip = check_flip_args(hm, flipped, shift, pairs, who)
    dark = check_decode_args(hm, decode, kernel, sigma, udp, refine, who)
    merged = _check_merged(merged, hm, flip, who)
    extra = ((flip[0],) if flip is not None else ()) + ((merged,) if isinstance(merged, torch.Tensor) else ())
    dev = _args.resolve_device((hm,) + parts + extra, device, who)
    if flip is None:
        return _decode(hm.to(dev), tuple(t.to(dev) for t in parts), kind, aspect, refine, h36m, dark=dark)
    if isinstance(merged, torch.Tensor) and any(t.is_cuda and t.numel() and _spans_overlap(t, merged) for t in (hm, flip[0])):
        raise ValueError(f"{who}: merged must not overlap heatmaps or flipped")
    flip = (flip[0].to(dev),) + flip[1:]
    if merged is None:
        return _decode(hm.to(dev), tuple(t.to(dev) for t in parts), kind, aspect, refine, h36m, flip, dark=dark)
    return FlipDecode(*_decode(hm.to(dev), tuple(t.to(dev) for t in parts), kind, aspect, refine, h36m, flip, merged, dark=dark))


def decode(hm: torch.Tensor, parts, kind: int, aspect: float, refine: bool, h36m: bool, flip=None, merged=None, dark=None):
    """``kasf_heatmap_keypoints`` on checked CUDA tensors of one device (what ``heatmaps_to_keypoints`` and ``StreamLifter.push_heatmaps`` end in); with
    ``flip`` = ``(hmf, shift, partner)`` of ``check_flip_args``, ``kasf_heatmap_flip_keypoints``, and with ``merged`` (True, or the checked tensor to
    fill) -> ``(keypoints, merged maps)``.  With ``dark`` = ``(mode, weights, udp)`` of ``check_decode_args``, ``kasf_heatmap_decode`` takes both cases."""
    if dark is not None:
        return _decode_dark(hm, parts, kind, aspect, h36m, flip, merged, dark)
    lead, (H, W) = tuple(hm.shape[:-3]), hm.shape[-2:]
    hm = hm.contiguous()                                         # the same tensor when it already is
    geom = (torch.cat(parts, dim=-1) if len(parts) == 2 else parts[0]).contiguous()
    out = torch.empty(lead + (17, 3), dtype=torch.float32, device=hm.device)
    n = out.numel() // 51
    if flip is None:
        if n:
            scratch = torch.empty_like(out) if h36m else None
            with torch.cuda.device(hm.device):
                _lib.check(_lib.load().kasf_heatmap_keypoints(hm.data_ptr(), _args.DTYPES[hm.dtype], n, int(H), int(W), geom.data_ptr(), kind, aspect,
                                                              int(bool(refine)), _lib.LAYOUT_H36M if h36m else _lib.LAYOUT_COCO, out.data_ptr(),
                                                              scratch.data_ptr() if h36m else None, _args.stream()))
        return out
    hmf, shift, partner = flip
    partner = np.ascontiguousarray(partner, dtype=np.int32)      # host memory, read during the call
    if partner.shape != (17,):
        raise ValueError(f"heatmap decode: the partner table must have 17 entries, got shape {partner.shape}")
    hmf = hmf.contiguous()
    if merged is True:
        merged = torch.empty(tuple(hm.shape), dtype=torch.float32, device=hm.device)
    if n:
        scratch = torch.empty_like(out) if h36m else None
        with torch.cuda.device(hm.device):
            _lib.check(_lib.load().kasf_heatmap_flip_keypoints(hm.data_ptr(), hmf.data_ptr(), _args.DTYPES[hm.dtype], n, int(H), int(W), partner.ctypes.data,
                                                               int(shift), geom.data_ptr(), kind, aspect, int(bool(refine)),
                                                               _lib.LAYOUT_H36M if h36m else _lib.LAYOUT_COCO, out.data_ptr(),
                                                               scratch.data_ptr() if h36m else None, merged.data_ptr() if merged is not None else None,
                                                               _args.stream()))
    return out if merged is None else (out, merged)


_decode = decode                 # heatmaps_to_keypoints' own ``decode`` argument shadows the function's name there


def _decode_dark(hm: torch.Tensor, parts, kind: int, aspect: float, h36m: bool, flip, merged, dark):
    """``decode`` through ``kasf_heatmap_decode``."""
    mode, weights, udp = dark
    lead, (H, W) = tuple(hm.shape[:-3]), hm.shape[-2:]
    hm = hm.contiguous()
    geom = (torch.cat(parts, dim=-1) if len(parts) == 2 else parts[0]).contiguous()
    out = torch.empty(lead + (17, 3), dtype=torch.float32, device=hm.device)
    n = out.numel() // 51
    hmf, shift, partner = (None, True, None) if flip is None else flip
    if flip is not None:
        partner = np.ascontiguousarray(partner, dtype=np.int32)  # host memory, read during the call
        if partner.shape != (17,):
            raise ValueError(f"heatmap decode: the partner table must have 17 entries, got shape {partner.shape}")
        hmf = hmf.contiguous()
        if merged is True:
            merged = torch.empty(tuple(hm.shape), dtype=torch.float32, device=hm.device)
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float32)  # host memory as well
    if n:
        scratch = torch.empty_like(out) if h36m else None
        with torch.cuda.device(hm.device):
            _lib.check(_lib.load().kasf_heatmap_decode(hm.data_ptr(), hmf.data_ptr() if flip is not None else None, _args.DTYPES[hm.dtype], n, int(H), int(W),
                                                       partner.ctypes.data if flip is not None else None, int(shift), geom.data_ptr(), kind, aspect, mode,
                                                       weights.ctypes.data if weights is not None else None, int(weights.size) if weights is not None else 1,
                                                       int(udp), _lib.LAYOUT_H36M if h36m else _lib.LAYOUT_COCO, out.data_ptr(),
                                                       scratch.data_ptr() if h36m else None, merged.data_ptr() if merged is not None else None, _args.stream()))
    return out if merged is None else (out, merged)
