"""The step behind everything else: the tracked skeletons painted over the uint8 BGR frame and the frame written as the NV12 surface a hardware encoder takes, on the GPU.

    res = draw_poses(frame, kp, valid, surface=True)           # frame uint8 [Hf,Wf,3] / [F,Hf,Wf,3], kp fp32 [P,J,2 or 3] / [F,P,J,2 or 3] in frame pixels
    res.frame, res.y, res.uv                                   # the painted frame (a new tensor; out=frame paints in place), the surface's two planes
    res = draw_poses(frame, kp, out=False, surface=(y, uv))    # the surface alone, into the encoder's own pitched planes
    y, uv = bgr_to_nv12(frame)                                 # no drawing: the inverse of yuv_to_bgr(y, uv)
    panel = poses_to_panel(world, rect=(1280, 0, 1920, 640))   # world-space poses [N,17,3] -> [N,17,2] pixels inside the rectangle: the 3-D plot's projection
    draw_poses(frame, panel, fills=[(1280, 0, 1920, 640, 255, 255, 255)], out=frame)

The demo shows its result with ``plot_on_frame`` (demo/demo.py:91-105: ``cv2.line`` and ``cv2.circle`` per bone on a host copy of the frame), draws only joints
above a score (demo/lib/hrnet/lib/utils/utilitys.py:24-58), plots the 3-D pose beside it with matplotlib (demo/demo.py:159-191) and hands the host frame to
``cv2.VideoWriter`` (demo/demo.py:307-323).  ``draw_poses`` is all of the 2-D part as one launch (csrc/k_draw.hip): opaque lines, dots and filled rectangles in
``plot_on_frame``'s order, and the painted pixels converted to NV12 on the way out.  include/kasf.h (``kasf_draw_poses``) states the rules: joints truncated
toward zero, exact integer Euclidean coverage, 20-bit fixed-point colour conversion with one table per matrix and range.  It is exact geometry, NOT OpenCV's
``ThickLine`` / midpoint circle: equality with cv2's drawing, or with a particular encoder's colour handling, is not claimed.  Text, anti-aliasing, alpha and
per-track colours are out of scope.
"""
from __future__ import annotations

import colorsys
import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _args, _lib
from ._args import pitched, step
from .yuv import MATRICES

# the 16 bones of the H36M tree as (child, parent) joint pairs: the model's own bone table (csrc/k_misc.hip, model/KASportsFormer.py:46-47)
H36M_SEGMENTS = tuple(zip((0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15), range(1, 17)))


def hue_wheel(n: int) -> np.ndarray:
    """The project's default palette: n fully saturated hues, evenly spaced from red, as uint8 [n,3] in B, G, R order."""
    rgb = [colorsys.hsv_to_rgb(i / max(n, 1), 1.0, 1.0) for i in range(n)]
    return np.array([[round(255 * b), round(255 * g), round(255 * r)] for r, g, b in rgb], np.uint8).reshape(n, 3)


class DrawResult(NamedTuple):
    frame: Optional[torch.Tensor]      # uint8 [Hf,Wf,3] / [F,Hf,Wf,3]: the painted frame (``out`` itself when given), or None with out=False
    y: Optional[torch.Tensor]          # uint8 [Hf,Wf] / [F,Hf,Wf]: the surface's luma plane, or None without a surface
    uv: Optional[torch.Tensor]         # uint8 [ch,cw,2] / [F,ch,cw,2]: its interleaved chroma plane


_consts: dict = {}


def _const(dev: torch.device, a: np.ndarray) -> torch.Tensor:
    """A small host table on the device, uploaded once per content: segments, colours and fills rarely change between frames."""
    key = (str(dev), a.dtype.str, a.shape, a.tobytes())
    t = _consts.get(key)
    if t is None:
        if len(_consts) >= 64:
            _consts.clear()
        t = _consts[key] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t


def _table(v, dtype, cols: int, who: str, name: str, most: int):
    """An [n, cols] table of small integers given as a list, numpy or a tensor -> a contiguous CUDA tensor as it is, or a checked numpy array to upload."""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        want = torch.int32 if dtype == np.int32 else torch.uint8
        if v.dtype != want or v.dim() != 2 or v.shape[1] != cols or v.shape[0] > most:
            raise ValueError(f"{who}: a CUDA {name} must be {want} [n <= {most}, {cols}], got {v.dtype} {tuple(v.shape)}")
        return v.detach().contiguous()
    a = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
    if a.size == 0:
        a = np.zeros((0, cols), dtype)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{who}: {name} must be integers, got {a.dtype}")
    if a.ndim != 2 or a.shape[1] != cols or a.shape[0] > most:
        raise ValueError(f"{who}: {name} must be [n <= {most}, {cols}], got {a.shape}")
    info = np.iinfo(dtype)
    if a.size and (a.min() < info.min or a.max() > info.max):
        raise ValueError(f"{who}: {name} has values outside {info.min}..{info.max}")
    return a.astype(dtype)


def _color3(v, who: str, name: str):
    a = np.asarray(v)
    if a.dtype.kind not in "iu" or a.shape != (3,):
        raise TypeError(f"{who}: {name} must be three integers, got {v!r}")
    if a.min() < 0 or a.max() > 255:
        raise ValueError(f"{who}: {name} must be in 0..255, got {v!r}")
    return (C.c_uint8 * 3)(*(int(x) for x in a))


def _out_plane(t, shape, who: str, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.uint8:
        raise TypeError(f"{who}: {name} must be uint8, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name} must be on a GPU, got {t.device}; kasportsformer_amd has no CPU path")
    return t.detach()


def check_draw_args(frame, keypoints, valid, segments, colors, dot_color, thickness, dot_radius, min_score, fills, out, surface, matrix, who: str):
    """Everything ``draw_poses`` can refuse without a device -> a dict of checked pieces (tensors where they are, tables as numpy or CUDA tensors)."""
    if matrix not in MATRICES:
        raise ValueError(f"{who}: matrix must be 'bt601' or 'bt709', got {matrix!r}")
    fr = _args.frames(frame, who)
    batched = fr.dim() == 4
    lead = tuple(fr.shape[:-3])
    Hf, Wf = int(fr.shape[-3]), int(fr.shape[-2])
    kp = None
    if keypoints is not None:
        if isinstance(keypoints, np.ndarray):
            keypoints = torch.from_numpy(np.ascontiguousarray(keypoints))
        if not isinstance(keypoints, torch.Tensor):
            raise TypeError(f"{who}: keypoints must be a numpy array or a torch tensor, got {type(keypoints).__name__}")
        if not keypoints.is_floating_point():
            raise TypeError(f"{who}: keypoints must be floating point, got {keypoints.dtype}")
        kp = keypoints.detach()
        if kp.dim() != len(lead) + 3 or tuple(kp.shape[:len(lead)]) != lead or kp.shape[-1] not in (2, 3) or not 1 <= kp.shape[-2] <= _lib.DRAW_MAX_JOINTS:
            raise ValueError(f"{who}: frame {tuple(fr.shape)} goes with keypoints {lead + ('P', 'J', '2 or 3')}, 1 <= J <= {_lib.DRAW_MAX_JOINTS}, got {tuple(kp.shape)}")
        if kp.shape[-3] > 1 << 20:
            raise ValueError(f"{who}: at most 2^20 persons, got {kp.shape[-3]}")
    P = 0 if kp is None else int(kp.shape[-3])
    va = None
    if valid is not None:
        if isinstance(valid, np.ndarray):
            valid = torch.from_numpy(np.ascontiguousarray(valid))
        if not isinstance(valid, torch.Tensor):
            raise TypeError(f"{who}: valid must be a numpy array or a torch tensor, got {type(valid).__name__}")
        if valid.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{who}: valid must be bool or uint8, got {valid.dtype}")
        if kp is None or tuple(valid.shape) != lead + (P,):
            raise ValueError(f"{who}: valid must be {lead + (P,)} (one flag per keypoint row), got {tuple(valid.shape)}")
        va = valid.detach()
    J = 0 if kp is None else int(kp.shape[-2])
    seg = _table(H36M_SEGMENTS if segments is None else segments, np.int32, 2, who, "segments", _lib.DRAW_MAX_SEGMENTS)
    S = int(seg.shape[0])
    if isinstance(seg, np.ndarray) and S and P and (seg.min() < 0 or seg.max() >= J):
        raise ValueError(f"{who}: segments name joints 0..{int(seg.max())}, the keypoints have J = {J}")
    col = _table(hue_wheel(S) if colors is None else colors, np.uint8, 3, who, "colors", _lib.DRAW_MAX_SEGMENTS)
    if int(col.shape[0]) != S:
        raise ValueError(f"{who}: {S} segments go with {S} colors, got {int(col.shape[0])}")
    fl = None if fills is None else _table(fills, np.int32, 7, who, "fills", _lib.DRAW_MAX_FILLS)
    if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float, np.floating, np.integer))):
        raise TypeError(f"{who}: min_score must be a number or None, got {type(min_score).__name__}")
    o = None
    if out is not None and out is not False:
        o = _out_plane(out, lead + (Hf, Wf, 3), who, "out")
        if not pitched(o if batched else o[None], 3):
            raise ValueError(f"{who}: out is written in place: its innermost two dimensions must be contiguous, its rows at least 3 * Wf bytes apart and its frames "
                             f"must not overlap, got strides {tuple(o.stride())}")
    sy = suv = None
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    if isinstance(surface, (tuple, list)):
        if len(surface) != 2:
            raise ValueError(f"{who}: surface must be True, False or the pair (y, uv)")
        sy = _out_plane(surface[0], lead + (Hf, Wf), who, "surface y")
        suv = _out_plane(surface[1], lead + (ch, cw, 2), who, "surface uv")
        if not pitched(sy if batched else sy[None], 1) or not pitched(suv if batched else suv[None], 2):
            raise ValueError(f"{who}: the surface is written in place: each plane's rows must be contiguous and at least a row apart, its frames must not overlap, "
                             f"got strides {tuple(sy.stride())} and {tuple(suv.stride())}")
    elif not isinstance(surface, (bool, np.bool_)):
        raise TypeError(f"{who}: surface must be True, False or the pair (y, uv), got {type(surface).__name__}")
    if out is False and not surface:
        raise ValueError(f"{who}: out=False leaves nothing to write without surface=True or surface=(y, uv)")
    return dict(frame=fr if batched else fr[None], kp=None if kp is None else (kp if batched else kp[None]), valid=None if va is None else (va if batched else va[None]),
                seg=seg, col=col, fills=fl, dot=_color3(dot_color, who, "dot_color"), t=_args.index_in(thickness, who, "thickness", 1, _lib.DRAW_MAX_THICKNESS),
                r=_args.index_in(dot_radius, who, "dot_radius", 0, _lib.DRAW_MAX_RADIUS), min_score=float("nan") if min_score is None else float(min_score),
                out=None if o is None else (o if batched else o[None]), want_out=out is not False,
                y=None if sy is None else (sy if batched else sy[None]), uv=None if suv is None else (suv if batched else suv[None]), want_surface=bool(surface),
                matrix=MATRICES[matrix], batched=batched)


def draw_poses(frame, keypoints, valid=None, *, segments=None, colors=None, dot_color=(255, 255, 255), thickness: int = 2, dot_radius: int = 2, min_score=None,
               fills=None, out=None, surface=False, matrix: str = "bt601", full_range: bool = False, rgb: bool = False, device=None) -> DrawResult:
    """Paint skeletons over a frame and / or write the painted frame as an NV12 surface, in one launch.

    ``frame`` uint8 [Hf,Wf,3] or [F,Hf,Wf,3], B, G, R (``rgb=True``: R, G, B): what ``nv12_to_bgr`` returns; read in place through its strides when a row's
    bytes are contiguous, never modified unless ``out`` is the frame.  ``keypoints`` fp32 [P,J,C] / [F,P,J,C], C = 2 (x, y) or 3 (x, y, score), in frame pixels, read
    through its strides as it is (a view of ``heatmaps_to_keypoints``' output or of the rows pushed to a ``TrackedLifter``); None draws no skeleton.  ``valid`` bool
    or uint8 [P] / [F,P] (``TrackedTick.valid``): rows that are drawn; None = all.  ``segments`` [S,2] joint pairs (default: the 16 bones of the H36M tree),
    ``colors`` [S,3] in the frame's channel order (default: ``hue_wheel(S)``), ``dot_color``, ``thickness`` 1..64, ``dot_radius`` 0..32 (0 = one pixel).
    ``min_score``: with C = 3, only joints whose score is above it are visible.  ``fills`` [R,7] = x0, y0, x1, y1, c0, c1, c2, R <= 8: rectangles painted
    before the skeletons (a panel's background).  Lists and numpy tables are uploaded once and kept; CUDA tensors are used as they are.

    ``out``: None = a new frame; a uint8 GPU tensor of the frame's shape (rows may be padded) is written in place -- ``out=frame`` paints the frame itself;
    False = no frame.  ``surface``: True = new planes, or the pair ``(y [..,Hf,Wf], uv [..,ch,cw,2])`` of views into the encoder's surface, written through their
    pitches.  ``matrix`` / ``full_range`` as ``yuv_to_bgr``.

    Returns ``DrawResult(frame, y, uv)``.  One launch, no host synchronisation, the same bits from run to run and for a frame alone or in a batch.  Rules:
    include/kasf.h, ``kasf_draw_poses`` (exact integer geometry; not cv2's rasteriser).  There is no host path: without a GPU the call raises ``RuntimeError``.
    Exception types as ``yuv_to_bgr``; every refusal comes before any launch."""
    who = "draw_poses"
    a = check_draw_args(frame, keypoints, valid, segments, colors, dot_color, thickness, dot_radius, min_score, fills, out, surface, matrix, who)
    tables = tuple(t for t in (a["seg"], a["col"], a["fills"]) if isinstance(t, torch.Tensor))
    dev = _args.resolve_device((a["frame"], a["kp"], a["valid"], a["out"], a["y"], a["uv"]) + tables, device, who)
    fr = a["frame"].to(dev)
    if not pitched(fr, 3):
        fr = fr.contiguous()
    res = paint(fr, None if a["kp"] is None else a["kp"].to(dev, torch.float32), None if a["valid"] is None else a["valid"].to(dev), a, bool(full_range), bool(rgb))
    if not a["batched"]:
        res = DrawResult(*(None if t is None else t[0] for t in res))
    return DrawResult(out if a["out"] is not None else res.frame, res.y if a["y"] is None else surface[0], res.uv if a["uv"] is None else surface[1])


def paint(fr: torch.Tensor, kp, valid, a: dict, full_range: bool, rgb: bool) -> DrawResult:
    """``kasf_draw_poses`` on checked CUDA tensors of one device: fr [F,Hf,Wf,3] pitched, kp [F,P,J,C] fp32 or None, valid [F,P] or None."""
    dev = fr.device
    F, Hf, Wf = (int(s) for s in fr.shape[:3])
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    seg, col, fl = (t if t is None or isinstance(t, torch.Tensor) else _const(dev, t) for t in (a["seg"], a["col"], a["fills"]))
    out, y, uv = a["out"], a["y"], a["uv"]
    if out is None and a["want_out"]:
        out = torch.empty((F, Hf, Wf, 3), dtype=torch.uint8, device=dev)
    if y is None and a["want_surface"]:
        y = torch.empty((F, Hf, Wf), dtype=torch.uint8, device=dev)
        uv = torch.empty((F, ch, cw, 2), dtype=torch.uint8, device=dev)
    if valid is not None and valid.dtype == torch.bool:
        valid = valid.view(torch.uint8)
    P, J, Cc = (0, 0, 0) if kp is None else (int(s) for s in kp.shape[1:])
    S, R = int(seg.shape[0]), 0 if fl is None else int(fl.shape[0])
    fs = (lambda t: int(t.stride(0)) if F > 1 else 0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().kasf_draw_poses(
            fr.data_ptr(), F, Hf, Wf, step(fr, 1, 3 * Wf), fs(fr),
            None if kp is None or P == 0 else kp.data_ptr(), P, J, Cc, *((0, 0, 0, 0) if kp is None else (int(s) for s in kp.stride())),
            None if valid is None or P == 0 else valid.data_ptr(), *((0, 0) if valid is None else (int(s) for s in valid.stride())),
            seg.data_ptr() if S else None, col.data_ptr() if S else None, S, a["dot"], a["t"], a["r"], a["min_score"], fl.data_ptr() if R else None, R,
            None if out is None else out.data_ptr(), 0 if out is None else step(out, 1, 3 * Wf), 0 if out is None else fs(out),
            None if y is None else y.data_ptr(), None if uv is None else uv.data_ptr(), 0 if y is None else step(y, 1, Wf), 0 if uv is None else step(uv, 1, 2 * cw),
            0 if y is None else fs(y), 0 if uv is None else fs(uv), a["matrix"], int(full_range), int(rgb), _args.stream()))
    return DrawResult(out, y, uv)


def bgr_to_nv12(frame, *, surface=True, matrix: str = "bt601", full_range: bool = False, rgb: bool = False, device=None):
    """The uint8 frame [Hf,Wf,3] / [F,Hf,Wf,3] -> its NV12 surface ``(y, uv)``: y [..,Hf,Wf], uv [..,(Hf + 1) // 2,(Wf + 1) // 2,2], new tensors or the pair
    given as ``surface`` (views into an encoder's pitched surface).  The inverse of ``yuv_to_bgr(y, uv)`` with the same ``matrix`` / ``full_range`` / ``rgb``:
    one chroma sample per 2 x 2 quad from the quad's mean.  ``kasf_bgr_to_nv12``: the ``draw_poses`` launch with nothing to paint."""
    a = check_draw_args(frame, None, None, (), (), (0, 0, 0), 1, 0, None, None, False, surface, matrix, "bgr_to_nv12")
    dev = _args.resolve_device((a["frame"], a["y"], a["uv"]), device, "bgr_to_nv12")
    fr = a["frame"].to(dev)
    if not pitched(fr, 3):
        fr = fr.contiguous()
    F, Hf, Wf = (int(s) for s in fr.shape[:3])
    y, uv = a["y"], a["uv"]
    if y is None:
        y = torch.empty((F, Hf, Wf), dtype=torch.uint8, device=dev)
        uv = torch.empty((F, (Hf + 1) // 2, (Wf + 1) // 2, 2), dtype=torch.uint8, device=dev)
    fs = (lambda t: int(t.stride(0)) if F > 1 else 0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().kasf_bgr_to_nv12(fr.data_ptr(), F, Hf, Wf, step(fr, 1, 3 * Wf), fs(fr), y.data_ptr(), uv.data_ptr(), step(y, 1, Wf),
                                                step(uv, 1, 2 * ((Wf + 1) // 2)), fs(y), fs(uv), a["matrix"], int(full_range), int(rgb), _args.stream()))
    if a["y"] is not None:
        return surface[0], surface[1]
    return (y, uv) if a["batched"] else (y[0], uv[0])


def panel_view(rect, elev: float = 5.0, azim: float = 5.0, radius: float = 0.72) -> np.ndarray:
    """The eight fp32 numbers ``kasf_pose_panel`` takes, formed in fp64 and rounded once (include/kasf.h): the orthographic view of matplotlib's
    ``view_init(elev, azim)`` into the panel ``rect = (x0, y0, x1, y1)``, ``radius`` world units from the root joint reaching half the panel's shorter side."""
    try:
        x0, y0, x1, y1 = (float(v) for v in rect)
    except (TypeError, ValueError):
        raise TypeError(f"poses_to_panel: rect must be four numbers (x0, y0, x1, y1), got {rect!r}") from None
    vals = (x0, y0, x1, y1, float(elev), float(azim), float(radius))
    if not all(math.isfinite(v) for v in vals) or x1 <= x0 or y1 <= y0 or radius <= 0:
        raise ValueError(f"poses_to_panel: rect must have x0 < x1 and y0 < y1, radius > 0, everything finite; got rect {rect!r}, elev {elev}, azim {azim}, radius {radius}")
    el, az = np.float64(math.radians(elev)), np.float64(math.radians(azim))
    right = np.array([-np.sin(az), np.cos(az), 0.0], np.float64)
    up = np.array([-np.sin(el) * np.cos(az), -np.sin(el) * np.sin(az), np.cos(el)], np.float64)
    scale = np.float64(min(x1 - x0, y1 - y0)) / 2.0 / np.float64(radius)
    return np.concatenate([scale * right, -scale * up, [(x0 + x1) / 2.0, (y0 + y1) / 2.0]]).astype(np.float32)


def poses_to_panel(world, rect, elev: float = 5.0, azim: float = 5.0, radius: float = 0.72, *, device=None) -> torch.Tensor:
    """World-space poses fp32 [...,17,3] (``poses_to_world``'s output) -> fp32 [...,17,2] pixel coordinates inside ``rect = (x0, y0, x1, y1)``, on the GPU: the
    projection of the demo's 3-D plot (demo/demo.py:159-191: ``view_init(elev, azim)``, +-``RADIUS`` = 0.72 around the root joint), orthographic.  The result is
    what ``draw_poses`` takes as keypoints, after a ``fills`` rectangle for the panel's background.  matplotlib's perspective camera, axes and ticks are out of
    scope.  One launch (``kasf_pose_panel``); the numpy restatement in fp32 gives the same bits."""
    who = "poses_to_panel"
    view = panel_view(rect, elev, azim, radius)
    if isinstance(world, np.ndarray):
        world = torch.from_numpy(np.ascontiguousarray(world))
    if not isinstance(world, torch.Tensor):
        raise TypeError(f"{who}: world must be a numpy array or a torch tensor, got {type(world).__name__}")
    if not world.is_floating_point():
        raise TypeError(f"{who}: world must be floating point, got {world.dtype}")
    if world.dim() < 2 or tuple(world.shape[-2:]) != (17, 3):
        raise ValueError(f"{who}: expected world [...,17,3], got {tuple(world.shape)}")
    dev = _args.resolve_device((world.detach(),), device, who)
    w = world.detach().to(dev, torch.float32).contiguous()
    out = torch.empty(tuple(w.shape[:-1]) + (2,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().kasf_pose_panel(w.data_ptr(), w.numel() // 51, view.ctypes.data_as(C.POINTER(C.c_float)), out.data_ptr(), _args.stream()))
    return out
