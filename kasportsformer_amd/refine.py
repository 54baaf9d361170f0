"""Recorded tracks cleaned up with the frames after a gap known, on the device: occlusion gaps filled and a zero-phase smoothing.

    kp = refine_tracks(kp_packed, offsets=offsets, min_score=0.3, max_gap=15, sigma=2.0)      # also a list of [N_i,J,Ct], one [N,J,Ct] or [P,N,J,Ct]
    kp, state = refine_tracks(tracks, return_state=True)      # state: uint8 [.., J], 0 usable, 1 interpolated, 2 held, 3 left as it came
    poses = refine_tracks(poses, score=False)                 # poses have no score: only a NaN or an infinity gates a joint

``smooth_tracks`` replays the live One-Euro filter over a file: a joint below ``min_score`` holds its last estimate, after ``max_hold`` frames it passes as it
came, and a causal filter lags.  A recorded track knows what comes after a gap.  Per (track, joint), include/kasf.h's rule (``kasf_tracks_refine``): a joint is
usable by the One-Euro filter's test (finite values, score at least ``min_score``); a joint that is not is interpolated linearly between its nearest usable
neighbours when the gap is at most ``max_gap`` frames, held at the nearest usable frame when it is in a leading or trailing run of at most ``max_gap`` frames,
and otherwise left as it came; then every joint that is usable or filled becomes a weighted mean over the usable and filled joints of a symmetric window,
``radius`` frames either way and narrower towards the ends of the track, with the weights ``w[k] = float32(exp(-k**2 / (2 * sigma**2)))`` computed here in
fp64 and rounded once -- the kernel calls no transcendental.  The score is copied through: a filled joint keeps its low score.

Parallel over frames, one launch, nothing read back, no host path.  ``sigma`` is in frames; the defaults are a starting point, not tuned on footage.  A live
form does not exist (a zero-phase filter needs the frames after; ``OneEuroFilter`` is the live stage), Savitzky-Golay coefficients are not built (the entry
takes any non-negative table), and the forms of recorded tracks are ``_tracks.py``'s, as for ``smooth_tracks``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in
from ._tracks import pack, recorded_parts, split, track_offsets
from .smooth import MAX_CHANNELS, MAX_JOINTS

MAX_GAP, MAX_RADIUS = 64, 32           # max_gap and radius of kasf_tracks_refine


def _track_rows(a, who: str) -> torch.Tensor:
    t = _args.as_tensor(a, who, "tracks", _args.FLOAT32)
    if t.dim() < 3:
        raise ValueError(f"{who}: expected tracks of [N,J,Ct], got {tuple(t.shape)}")
    return t


def gaussian_table(sigma, radius) -> np.ndarray:
    """``w[k] = float32(exp(-k**2 / (2 * sigma**2)))`` for k = 0 .. radius, computed in fp64 and rounded once; zeros above ``radius``.  fp32 [33]."""
    w = np.zeros(MAX_RADIUS + 1, np.float32)
    k = np.arange(radius + 1, dtype=np.float64)
    w[:radius + 1] = np.exp(-k * k / (2.0 * float(sigma) ** 2)).astype(np.float32) if radius else 1.0
    return w


def refine_params(min_score=0.3, max_gap=15, sigma=2.0, radius=None, who: str = "refine_tracks") -> _lib.KasfRefineParams:
    """The parameters as the entry point takes them, refused as the entry point refuses them.  ``radius=None``: ``min(32, ceil(3 * sigma))``; ``sigma=None``:
    radius 0, the gap fill alone."""
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: min_score must be a number, got {type(min_score).__name__}")
    if not np.isfinite(np.float32(min_score)):
        raise ValueError(f"{who}: min_score must be finite, got {min_score}")
    max_gap = index_in(max_gap, who, "max_gap", 0, MAX_GAP)
    if sigma is None:
        if radius not in (None, 0):
            raise ValueError(f"{who}: sigma=None is the gap fill alone (radius 0), got radius={radius}")
        radius = 0
    else:
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)):
            raise TypeError(f"{who}: sigma must be a number of frames or None, got {type(sigma).__name__}")
        if not (np.isfinite(sigma) and 1e-3 <= float(sigma) <= 1e3):
            raise ValueError(f"{who}: sigma must be in [1e-3, 1e3] frames, got {sigma}")
        radius = min(MAX_RADIUS, math.ceil(3.0 * float(sigma))) if radius is None else index_in(radius, who, "radius", 0, MAX_RADIUS)
    w = gaussian_table(1.0 if sigma is None else sigma, radius)
    return _lib.KasfRefineParams(float(min_score), max_gap, radius, (C.c_float * (MAX_RADIUS + 1))(*w.tolist()))


def refine_tracks(tracks, offsets=None, *, score: bool = True, min_score: float = 0.3, max_gap: int = 15, sigma=2.0, radius=None, return_state: bool = False,
                  device=None):
    """Recorded tracks with their occlusion gaps filled and a zero-phase Gaussian over what is known, in one launch; see the module docstring.  ``tracks``: a
    sequence of [N_i,J,Ct] float32 arrays (numpy or torch, on the host or the GPU, any N_i >= 0, never modified) -> a list of CUDA fp32 [N_i,J,Ct], views of one
    packed result; with ``offsets`` (integers [P+1] as ``lift_tracks`` takes them) one packed [sum N_i,J,Ct] array -> one packed tensor; one array [N,J,Ct] (a
    track) or [P,N,J,Ct] (P tracks of one length) -> its shape.  ``score``: the last of the Ct values is the score (keypoints; ``False`` for poses, where only a
    NaN or an infinity gates a joint).  ``max_gap`` in [0, 64] frames (0 fills nothing); ``sigma`` in frames, ``None`` for the gap fill alone; ``radius`` in
    [0, 32], ``None`` for ``min(32, ceil(3 * sigma))``.  ``return_state=True`` -> ``(tracks, state)``, the state uint8 [..,J] in the same form: 0 usable,
    1 interpolated, 2 held, 3 left as it came.  The defaults are a starting point, not tuned on footage.  Every refusal is raised before any launch."""
    who = "refine_tracks"
    params = refine_params(min_score, max_gap, sigma, radius, who)
    for name, v in (("score", score), ("return_state", return_state)):
        if not isinstance(v, (bool, np.bool_)):
            raise TypeError(f"{who}: {name} must be a bool, got {type(v).__name__}")
    parts, as_list = recorded_parts(tracks, offsets, who, lambda a: _track_rows(a, who), "J,Ct", True)
    if as_list and not parts:
        return ([], []) if return_state else []
    J, Ct = int(parts[0].shape[-2]), int(parts[0].shape[-1])
    if any(tuple(a.shape[-2:]) != (J, Ct) for a in parts):
        raise ValueError(f"{who}: every track must have the same [J,Ct], got {[tuple(a.shape) for a in parts]}")
    Cn = Ct - (1 if score else 0)
    if not 1 <= J <= MAX_JOINTS or not 1 <= Cn <= MAX_CHANNELS:
        raise ValueError(f"{who}: need J in [1, {MAX_JOINTS}] and {'Ct - 1' if score else 'Ct'} in [1, {MAX_CHANNELS}], got rows [{J},{Ct}]")
    off = track_offsets(parts, offsets, as_list, who)
    dev = _args.resolve_device(parts, device, who)
    packed = pack(parts, as_list, dev)
    out = torch.empty_like(packed)
    state = torch.empty(packed.shape[:-1], dtype=torch.uint8, device=dev) if return_state else None
    P, N = len(off) - 1, int(off[-1])
    if P > 0 and N > 0:
        off_d = torch.from_numpy(off).to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kasf_tracks_refine(packed.data_ptr(), off_d.data_ptr(), N, P, J, Cn, int(score), C.byref(params), out.data_ptr(),
                                                      state.data_ptr() if return_state else None, _args.stream()))
    if not return_state:
        return split(out, off) if as_list else out
    return (split(out, off), split(state, off)) if as_list else (out, state)
