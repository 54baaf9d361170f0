"""The step in front of everything else: a decoder's YUV 4:2:0 surface converted to the uint8 BGR frame ``letterbox_frames`` and ``crop_persons`` take, on the GPU.

    frame = nv12_to_bgr(surface)                               # surface uint8 [rows, pitch] on the GPU: Hf luma rows, then (Hf + 1) / 2 rows of U, V pairs
    frame = nv12_to_bgr(surface, 1080, 1920, chroma_row=1088)  # a 1080p surface whose height the decoder aligned to 1088, behind a pitch of 2048
    frame = i420_to_bgr(surface)                               # planar: Hf luma rows, then the U plane, then the V plane (FFmpeg's yuv420p in one buffer)
    frame = yuv_to_bgr(y, uv)                                  # the planes given one by one: y [Hf,Wf], uv [ch,cw,2]; layout="i420": yuv_to_bgr(y, u, v, layout="i420")
    lb = letterbox_frames(frame, inp_dim=416)

The demo gets its BGR frame from ``cv2.VideoCapture(video).read()`` (demo/lib/hrnet/gen_kpts.py:106,118): a host decode and a host conversion.  A hardware
decoder (VCN through rocDecode or VA-API) leaves NV12 surfaces in device memory, a software decoder planar I420; ``yuv_to_bgr`` is the conversion as one
launch (csrc/k_yuv.hip) that reads the surface in place through its pitch and writes the frame on the device -- also into a caller's pitched ``out=``.
include/kasf.h (``kasf_yuv420_to_bgr``) states the rule: nearest chroma siting, integers with 20 fractional bits, one coefficient table per matrix
(BT.601, BT.709) and range (limited, full), BT.601 limited being OpenCV's published constants.  It restates the documented fixed-point scheme of OpenCV's
portable ``cvtColor`` for 4:2:0 input; what ``cv2.VideoCapture.read()`` returns additionally depends on the FFmpeg build behind it.  There is no OpenCV
here: equality with a particular cv2 / FFmpeg build is NOT verified.
"""
from __future__ import annotations

import torch

from . import _args, _lib
from ._args import pitched, step

MAX_SIDE = _args.MAX_SIDE       # Hf, Wf the entry point takes
LAYOUTS = {"nv12": _lib.YUV_NV12, "i420": _lib.YUV_I420}
MATRICES = {"bt601": _lib.YUV_BT601, "bt709": _lib.YUV_BT709}


def check_yuv_args(y, u_or_uv, v, layout, matrix, out, who: str):
    """Everything ``yuv_to_bgr`` can refuse without a device -> ``(y, c0, c1 or None, layout code, matrix code, out or None, batched)`` with the planes as
    detached tensors where they are: y [F,Hf,Wf], c0 [F,ch,cw,2] (NV12) or c0, c1 [F,ch,cw] (I420)."""
    if layout not in LAYOUTS:
        raise ValueError(f"{who}: layout must be 'nv12' or 'i420', got {layout!r}")
    if matrix not in MATRICES:
        raise ValueError(f"{who}: matrix must be 'bt601' or 'bt709', got {matrix!r}")
    nv12 = layout == "nv12"
    if nv12 and v is not None:
        raise ValueError(f"{who}: layout 'nv12' takes the interleaved UV plane alone, not a separate v")
    if not nv12 and v is None:
        raise ValueError(f"{who}: layout 'i420' takes the U plane and the V plane")
    named = ((y, "y"), (u_or_uv, "uv")) if nv12 else ((y, "y"), (u_or_uv, "u"), (v, "v"))
    yt, *planes = (_args.as_tensor(p, who, name, _args.UINT8, keep_pitch=True) for p, name in named)
    if yt.dim() not in (2, 3) or not 1 <= yt.shape[-1] <= MAX_SIDE or not 1 <= yt.shape[-2] <= MAX_SIDE or (yt.dim() == 3 and yt.shape[0] < 1):
        raise ValueError(f"{who}: expected y [Hf,Wf] or [F,Hf,Wf] with F >= 1 and Hf, Wf in [1, {MAX_SIDE}], got {tuple(yt.shape)}")
    batched = yt.dim() == 3
    lead = tuple(yt.shape[:-2])
    Hf, Wf = int(yt.shape[-2]), int(yt.shape[-1])
    want = lead + ((Hf + 1) // 2, (Wf + 1) // 2) + ((2,) if nv12 else ())
    for name, p in zip(("uv",) if nv12 else ("u", "v"), planes):
        if tuple(p.shape) != want:
            raise ValueError(f"{who}: y {tuple(yt.shape)} goes with {name} {want} (4:2:0: (Hf + 1) / 2 rows of (Wf + 1) / 2 samples), got {tuple(p.shape)}")
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError(f"{who}: out must be a torch tensor, got {type(out).__name__}")
        if out.dtype != torch.uint8:
            raise TypeError(f"{who}: out must be uint8, got {out.dtype}")
        if tuple(out.shape) != lead + (Hf, Wf, 3):
            raise ValueError(f"{who}: y {tuple(yt.shape)} goes with out {lead + (Hf, Wf, 3)}, got {tuple(out.shape)}")
        if not out.is_cuda:
            raise RuntimeError(f"{who}: out must be on a GPU, got {out.device}; kasportsformer_amd has no CPU path")
        if not pitched(out if batched else out[None], 3):
            raise ValueError(f"{who}: out is written in place: its innermost two dimensions must be contiguous, its rows at least 3 * Wf bytes apart and its "
                             f"frames must not overlap, got strides {tuple(out.stride())}")
        out = out.detach()
    if not batched:
        yt, planes, out = yt[None], [p[None] for p in planes], None if out is None else out[None]
    return yt, planes[0], None if nv12 else planes[1], LAYOUTS[layout], MATRICES[matrix], out, batched


def yuv_to_bgr(y, u_or_uv, v=None, *, layout: str = "nv12", matrix: str = "bt601", full_range: bool = False, rgb: bool = False, out=None,
               device=None) -> torch.Tensor:
    """YUV 4:2:0 planes -> the uint8 BGR frame: ``y`` [Hf,Wf]; ``u_or_uv`` the interleaved plane [ch,cw,2] (``layout="nv12"``: U, V pairs) or the U plane
    [ch,cw] with ``v`` [ch,cw] (``layout="i420"``), ``ch = (Hf + 1) // 2``, ``cw = (Wf + 1) // 2`` -- odd sizes are legal, the last column / row shares the
    last chroma sample; or all of them with a leading ``F``.  A torch tensor on the GPU is the normal case: read in place, also as a strided view of a
    decoder's surface with padded rows, as long as a row's samples are contiguous (any other view is packed first; the U and V planes of I420 are read in
    place when their strides agree), never modified; numpy / torch on the host is uploaded.

    ``matrix``: "bt601" or "bt709"; ``full_range``: False = limited (16..235 / 16..240, what video carries), True = full (JPEG).  The default, BT.601
    limited, is the table of ``cv2.cvtColor(..., COLOR_YUV2BGR_NV12 / _I420)``.  ``rgb``: channels R, G, B instead of B, G, R.  ``out``: a uint8 GPU
    tensor [Hf,Wf,3] / [F,Hf,Wf,3] to write in place of a new one, through its own strides (innermost two dimensions contiguous, rows may be padded: every
    payload byte is written, no padding byte is).  ``device``: where host input goes (default: the current GPU); GPU input stays where it is.

    Returns the frame, uint8 [Hf,Wf,3] or [F,Hf,Wf,3] on the GPU (``out`` itself when given): what ``letterbox_frames`` and ``crop_persons`` take.  One
    launch, no host synchronisation, the same bits from run to run and for a frame alone or in a batch.  Arithmetic: include/kasf.h,
    ``kasf_yuv420_to_bgr`` (nearest chroma, 20-bit fixed point); not verified against a cv2 / FFmpeg build.  There is no host path: without a GPU the call
    raises ``RuntimeError``.  Exception types as ``crop_persons``; every refusal comes before any launch."""
    who = "yuv_to_bgr"
    yt, c0, c1, lay, mat, o, batched = check_yuv_args(y, u_or_uv, v, layout, matrix, out, who)
    dev = _args.resolve_device((yt, c0, c1, o), device, who)
    res = convert(yt.to(dev), c0.to(dev), None if c1 is None else c1.to(dev), lay, mat, bool(full_range), bool(rgb), o)
    return out if out is not None else (res if batched else res[0])


def convert(y: torch.Tensor, c0: torch.Tensor, c1, layout: int, matrix: int, full_range: bool, rgb: bool, out) -> torch.Tensor:
    """``kasf_yuv420_to_bgr`` on checked CUDA planes of one device: y [F,Hf,Wf], c0 [F,ch,cw,2] or c0, c1 [F,ch,cw]; out [F,Hf,Wf,3] or None."""
    F, Hf, Wf = (int(s) for s in y.shape)
    if not pitched(y, 1):
        y = y.contiguous()
    if c1 is None:
        if not pitched(c0, 2):
            c0 = c0.contiguous()
        c_row, c_frame = step(c0, -3, 2 * int(c0.shape[-2])), int(c0.stride(0))
    else:
        if not (pitched(c0, 1) and pitched(c1, 1) and (c0.shape[-2] == 1 or c0.stride(-2) == c1.stride(-2)) and (F == 1 or c0.stride(0) == c1.stride(0))):
            c0, c1 = c0.contiguous(), c1.contiguous()                       # the entry point takes one row stride and one frame stride for both planes
        c_row, c_frame = step(c0, -2, int(c0.shape[-1])), int(c0.stride(0))
    if out is None:
        out = torch.empty((F, Hf, Wf, 3), dtype=torch.uint8, device=y.device)
    y_frame, o_frame = int(y.stride(0)), int(out.stride(0))
    if F == 1:
        y_frame = c_frame = o_frame = 0
    with torch.cuda.device(y.device):
        _lib.check(_lib.load().kasf_yuv420_to_bgr(y.data_ptr(), c0.data_ptr(), None if c1 is None else c1.data_ptr(), layout, F, Hf, Wf, step(y, -2, Wf),
                                                  c_row, y_frame, c_frame, out.data_ptr(), step(out, -3, 3 * Wf), o_frame, matrix, int(full_range), int(rgb),
                                                  _args.stream()))
    return out


def surface_planes(surface, height, width, chroma_row, layout: str, who: str):
    """The planes inside a decoder's single allocation, as views (no device needed): ``surface`` uint8 [rows, pitch] or [F, rows, pitch] -> ``(y, uv)`` for
    "nv12", ``(y, u, v)`` for "i420"."""
    s = _args.as_tensor(surface, who, "surface", _args.UINT8, keep_pitch=True)
    if s.dim() not in (2, 3) or s.shape[-1] < 1 or s.shape[-2] < 1 or (s.dim() == 3 and s.shape[0] < 1):
        raise ValueError(f"{who}: expected surface [rows, pitch] or [F, rows, pitch], got {tuple(s.shape)}")
    rows, pitch = int(s.shape[-2]), int(s.shape[-1])
    Hf = rows * 2 // 3 if height is None else _args.index_in(height, who, "height", any_index=True)
    Wf = pitch if width is None else _args.index_in(width, who, "width", any_index=True)
    cr = Hf if chroma_row is None else _args.index_in(chroma_row, who, "chroma_row", any_index=True)
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    if not (1 <= Hf <= MAX_SIDE and 1 <= Wf <= MAX_SIDE):
        raise ValueError(f"{who}: height and width must be in [1, {MAX_SIDE}], got {Hf} x {Wf}")
    if cr < Hf:
        raise ValueError(f"{who}: chroma_row {cr} lies inside the {Hf} luma rows")
    if layout == "nv12":
        if Wf > pitch or 2 * cw > pitch or rows < cr + ch:
            raise ValueError(f"{who}: a {Hf} x {Wf} NV12 frame with its chroma at row {cr} needs a surface of at least {cr + ch} rows of {2 * cw} bytes, got "
                             f"{tuple(s.shape)}")
        return s[..., :Hf, :Wf], s[..., cr:cr + ch, :2 * cw].unflatten(-1, (cw, 2))
    if Hf % 2 or Wf % 2 or pitch % 2:
        raise ValueError(f"{who}: a packed I420 surface has even height, width and pitch (its chroma rows are half a luma row), got {Hf} x {Wf}, pitch {pitch}")
    if Wf > pitch or rows < cr + ch:
        raise ValueError(f"{who}: a {Hf} x {Wf} I420 frame with its chroma at row {cr} needs a surface of at least {cr + ch} rows of {Wf} bytes, got "
                         f"{tuple(s.shape)}")
    if s.stride(-1) != 1 or s.stride(-2) != pitch:
        s = s.contiguous()                                       # the chroma rows are half rows of the surface: they need its bytes in one piece
    half = pitch // 2
    flat = s.flatten(-2)
    u = flat[..., cr * pitch:cr * pitch + ch * half].unflatten(-1, (ch, half))[..., :cw]
    v = flat[..., cr * pitch + ch * half:cr * pitch + 2 * ch * half].unflatten(-1, (ch, half))[..., :cw]
    return s[..., :Hf, :Wf], u, v


def nv12_to_bgr(surface, height=None, width=None, *, chroma_row=None, matrix: str = "bt601", full_range: bool = False, rgb: bool = False, out=None,
                device=None) -> torch.Tensor:
    """An NV12 surface as a decoder hands it over -> the BGR frame: ``surface`` uint8 [rows, pitch] (or [F, rows, pitch]), ``height`` luma rows of ``width``
    samples followed by ``(height + 1) // 2`` rows of U, V pairs, every row ``pitch`` bytes apart -- also the shape of PyAV's ``to_ndarray(format="nv12")``.
    ``height`` defaults to ``rows * 2 // 3``, ``width`` to the pitch; ``chroma_row`` is the UV plane's first row where the decoder aligned the surface height
    (default: ``height``).  The planes are views of the surface: nothing is copied on the GPU.  Everything else as ``yuv_to_bgr``."""
    y, uv = surface_planes(surface, height, width, chroma_row, "nv12", "nv12_to_bgr")
    return yuv_to_bgr(y, uv, layout="nv12", matrix=matrix, full_range=full_range, rgb=rgb, out=out, device=device)


def i420_to_bgr(surface, height=None, width=None, *, chroma_row=None, matrix: str = "bt601", full_range: bool = False, rgb: bool = False, out=None,
                device=None) -> torch.Tensor:
    """A planar I420 surface (FFmpeg's ``yuv420p`` in one buffer, PyAV's ``to_ndarray(format="yuv420p")``) -> the BGR frame: ``surface`` uint8 [rows, pitch]
    (or [F, rows, pitch]), ``height`` luma rows, then from ``chroma_row`` (default: ``height``) the U plane as ``height // 2`` rows of ``pitch // 2`` bytes and
    the V plane right behind it.  That packing needs even ``height``, ``width`` and pitch.  ``height`` defaults to ``rows * 2 // 3``, ``width`` to the pitch.
    Everything else as ``yuv_to_bgr``."""
    y, u, v = surface_planes(surface, height, width, chroma_row, "i420", "i420_to_bgr")
    return yuv_to_bgr(y, u, v, layout="i420", matrix=matrix, full_range=full_range, rgb=rgb, out=out, device=device)
