"""Host-side argument plumbing the video and pose ops share: one definition each of what every public call does to its arguments before a launch.

Everything here is refused or resolved without touching a device, except ``stream()`` and the current-device lookup of ``resolve_device``.
"""
from __future__ import annotations

import ctypes as C
import operator

import numpy as np
import torch

from . import _lib

DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}     # the element types the entry points take
NP_DTYPES = (np.float32, np.float16)                # their numpy counterparts (numpy has no bfloat16)
FLOAT32, UINT8 = (torch.float32,), (torch.uint8,)
MAX_SIDE = 32767                                    # Hf, Wf of a frame the entry points take

_NUMPY = {torch.float32: np.float32, torch.float16: np.float16, torch.uint8: np.uint8}


def stream():
    """The current stream as the ``void*`` the entry points take."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def as_tensor(a, who: str, name: str, dtypes, keep_pitch: bool = False) -> torch.Tensor:
    """A numpy array (shared, not copied) or torch tensor of one of the torch ``dtypes``, on the host or a GPU, as a detached tensor where it is.  A strided
    numpy array is packed; with ``keep_pitch`` only one with a negative stride is, so that a decoder's padded pitch survives."""
    names = [str(d)[len("torch."):] for d in dtypes]
    want = names[0] if len(names) == 1 else ", ".join(names[:-1]) + " or " + names[-1]
    if isinstance(a, np.ndarray):
        if a.dtype not in [_NUMPY[d] for d in dtypes if d in _NUMPY]:
            raise TypeError(f"{who}: {name} must be {want}, got {a.dtype}")
        return torch.from_numpy(a if keep_pitch and all(s >= 0 for s in a.strides) else np.ascontiguousarray(a))
    if isinstance(a, torch.Tensor):
        if a.dtype not in dtypes:
            raise TypeError(f"{who}: {name} must be {want}, got {a.dtype}")
        if a.device.type not in ("cpu", "cuda"):
            raise RuntimeError(f"{who}: {name} on unsupported device {a.device}")
        return a.detach()
    raise TypeError(f"{who}: {name} must be a numpy array or a torch tensor, got {type(a).__name__}")


def frames(a, who: str) -> torch.Tensor:
    """uint8 frames [Hf,Wf,3] or [F,Hf,Wf,3], as ``as_tensor`` gives them with their pitch kept."""
    t = as_tensor(a, who, "frame", UINT8, keep_pitch=True)
    if t.dim() not in (3, 4) or t.shape[-1] != 3 or not 1 <= t.shape[-2] <= MAX_SIDE or not 1 <= t.shape[-3] <= MAX_SIDE or (t.dim() == 4 and t.shape[0] < 1):
        raise ValueError(f"{who}: expected frame [Hf,Wf,3] or [F,Hf,Wf,3] with F >= 1 and Hf, Wf in [1, {MAX_SIDE}], got {tuple(t.shape)}")
    return t


def resolve_device(tensors, device, who: str) -> torch.device:
    """Where a call runs, with an index: ``device=`` when given (it must be a GPU), else the GPU the tensors are on, else the current GPU; ``RuntimeError``
    without one, and when a GPU tensor (entries that are None are skipped) lives elsewhere."""
    on_gpu = [t.device for t in tensors if t is not None and t.is_cuda]
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
        raise RuntimeError(f"{who}: tensors on {sorted({str(d) for d in on_gpu})}, asked for {dev}")
    return dev


def index_in(v, who: str, name: str, lo=None, hi=None, any_index: bool = False) -> int:
    """An integer that is not a bool, in [lo, hi] when the bounds are given.  Two acceptance rules are in use and both stay: a Python or numpy integer
    (the default), or with ``any_index`` whatever ``operator.index`` takes."""
    try:
        if isinstance(v, bool) or not (any_index or isinstance(v, (int, np.integer))):
            raise TypeError
        v = operator.index(v)
    except TypeError:
        raise TypeError(f"{who}: {name} must be an int, got {repr(v) if isinstance(v, bool) else type(v).__name__}") from None
    if lo is not None and not lo <= v <= hi:
        raise ValueError(f"{who}: {name} must be in [{lo}, {hi}], got {v}")
    return v


def number(v, who: str, name: str) -> float:
    """A Python or numpy real number that is not a bool and is finite as the float32 an entry point takes."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: {name} must be a number, got {type(v).__name__}")
    if not np.isfinite(np.float32(v)):
        raise ValueError(f"{who}: {name} must be finite, got {v}")
    return float(v)


def step(p: torch.Tensor, dim: int, least: int) -> int:
    """The stride of dimension dim in bytes; a dimension of one element has no stride to speak of, so the least legal one stands in for it."""
    return int(p.stride(dim)) if p.shape[dim] > 1 else max(int(p.stride(dim)), least)


def pitched(p: torch.Tensor, inner: int) -> bool:
    """Can a kernel address the uint8 plane p -- [F,rows,cols] for inner = 1, [F,rows,cols,inner] otherwise -- through a row and a frame stride: a row's bytes
    contiguous, rows and frames not overlapping?  (Dimensions of one element are not looked at.)"""
    if inner > 1 and p.stride(-1) != 1:
        return False
    col, row = (-1, -2) if inner == 1 else (-2, -3)
    row_bytes = int(p.shape[col]) * inner
    return ((p.shape[col] == 1 or p.stride(col) == inner) and (p.shape[row] == 1 or p.stride(row) >= row_bytes) and
            (p.shape[0] == 1 or p.stride(0) >= int(p.shape[row]) * step(p, row, row_bytes)))
