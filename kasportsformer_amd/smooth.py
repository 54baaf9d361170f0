"""Steady keypoints and poses over time, on the device: the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) with its state next to the lifter's.

    f2 = OneEuroFilter(slots=32, joints=17, channels=2, score=True, rate=30.0, min_cutoff=1.0, beta=0.01, d_cutoff=1.0,
                       min_score=0.3, max_hold=15, device=model_device)
    kp = f2.push(kp)                            # [slots,17,3] -> the same shape, CUDA fp32; f2.push(kp, slots=[3, 7, 8]) as StreamLifter.push
    f2.reset(slots=[7])                         # the player left: the slot starts again
    ft = OneEuroFilter(streams=B, track_slots=S_t, rows="persons", num_person=P, ...)     # tracker-driven: TrackedLifter's constructor words
    kp = ft.push(kp, t); out = lifter.push(kp, t); poses = f3.push(out.poses, t)          # t: this tick's TrackResult, read in place; f3: channels=3, score=False
    ft.reset(streams=None)                      # goes with SortTracker.reset, like TrackedLifter.reset
    kp = smooth_tracks(kp_packed, offsets=offsets, ...)       # recorded tracks; also a list of [N_i,J,Ct], one [N,J,Ct] or [P,N,J,Ct]

``heatmaps_to_keypoints`` decodes every frame on its own, the lifters store a joint with score 0.05 like a good one, and consecutive poses of a sliding window
are unrelated: nothing ties one tick to the next.  This is what live pose pipelines put there.  A *row* is one person's frame ``[J, Ct]``: ``channels``
filtered values per joint and, with ``score``, the score behind them (keypoints: 17 x (x, y, score); poses: 17 x (x, y, z)).  Per joint, include/kasf.h's rule
(``kasf_one_euro_push``): a joint is usable when its values are finite and its score is at least ``min_score``; the first usable sample is passed through and
becomes the estimate; a joint that is not usable gets the estimate (it holds) for up to ``max_hold`` missed ticks, after which the estimate is dropped and the
input passes as it came; a usable joint moves the estimate by the One-Euro step with ``dt = ticks since its last update / rate``.  The score is copied through.

The state (``xhat``, ``dxhat`` [S,J,C], ``last`` [S,J] int64, ``owner`` [S] int32) is on the device and allocated once; the object keeps the tick as a host
integer, +1 per push (``ticks=n`` for a push after n - 1 dropped frames).  Nothing synchronises with the host and nothing is read back: one launch per push.
There is no host path.  The parameters are in the units of the data (pixels for keypoints, model units for poses); the defaults are a starting point, not
tuned on footage.  Per-person normalisation of ``beta`` is out of scope.

A tracker-driven filter resolves its rows by ``TrackedLifter``'s rule, which is one device function (``csrc/tracked_rows.h``); slot ids, stream indices, the
forms of recorded tracks and ``reset`` are handled by ``_tracks.py``, the layer the lifters and ``BoneLengthFilter`` use as well.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in
from ._tracks import check_push, filter_slots, pack, recorded_parts, reset_filter, split, track_offsets
from ._tracks import slot_ids as check_slot_ids, stream_ids as check_stream_ids     # noqa: F401 -- the names these two are known by here

MAX_JOINTS, MAX_CHANNELS, MAX_HOLD = 256, 4, 1 << 20       # J, C and max_hold of the kasf_one_euro_* entries
_LO, _HI = np.float32(1e-6), np.float32(1e6)


def one_euro_params(rate=30.0, min_cutoff=1.0, beta=0.01, d_cutoff=1.0, min_score=0.3, max_hold=15, who: str = "OneEuroFilter") -> _lib.KasfOneEuroParams:
    """The filter's parameters as the entry points take them (fp32; ``dt = 1 / rate`` rounded once), refused as the entry points refuse them."""
    vals = {}
    for name, v in (("rate", rate), ("min_cutoff", min_cutoff), ("beta", beta), ("d_cutoff", d_cutoff), ("min_score", min_score)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError(f"{who}: {name} must be a number, got {type(v).__name__}")
        vals[name] = float(v)
    if not vals["rate"] > 0 or not np.isfinite(vals["rate"]):
        raise ValueError(f"{who}: rate must be positive and finite, got {rate}")
    dt = np.float32(1.0 / vals["rate"])
    for name, v in (("1 / rate", dt), ("min_cutoff", np.float32(vals["min_cutoff"])), ("d_cutoff", np.float32(vals["d_cutoff"]))):
        if not _LO <= v <= _HI:
            raise ValueError(f"{who}: {name} must be in [1e-6, 1e6], got {v}")
    if not np.float32(0) <= np.float32(vals["beta"]) <= _HI:
        raise ValueError(f"{who}: beta must be in [0, 1e6], got {beta}")
    if not np.isfinite(np.float32(vals["min_score"])):
        raise ValueError(f"{who}: min_score must be finite, got {min_score}")
    max_hold = index_in(max_hold, who, "max_hold", 0, MAX_HOLD)
    return _lib.KasfOneEuroParams(float(dt), vals["min_cutoff"], vals["d_cutoff"], vals["beta"], vals["min_score"], max_hold)


def check_filter_args(slots, joints, channels, score, streams, track_slots, rows, num_person, who: str = "OneEuroFilter"):
    """Everything the constructor can refuse about its shape without a device -> ``(tracked, S, J, C, Ct, streams, track_slots, rows mode, R)``; the last four
    are None for a filter driven by slot ids."""
    J = index_in(joints, who, "joints", 1, MAX_JOINTS)
    Cn = index_in(channels, who, "channels", 1, MAX_CHANNELS)
    if not isinstance(score, (bool, np.bool_)):
        raise TypeError(f"{who}: score must be a bool, got {type(score).__name__}")
    tracked, S, *driven = filter_slots(slots, streams, track_slots, rows, num_person, who)
    return (tracked, S, J, Cn, Cn + (1 if score else 0), *driven)


class OneEuroFilter:
    """The One-Euro filter over the rows of a live pipeline with its state on the device; see the module docstring.  Built with ``slots=`` it is driven by host
    slot ids like ``StreamLifter``; built with ``streams=`` / ``track_slots=`` / ``rows=`` / ``num_person=`` (``TrackedLifter``'s words) it reads the slot, the
    births and the deaths of every row from this tick's ``TrackResult`` on the device, by the lifter's rule, so a filter and a lifter given the same result
    agree on whose history a row continues.  ``device``: the GPU (default: the current one).  The default parameters are a starting point, not tuned on
    footage.  Every refusal is raised before any launch and leaves the state and the tick as they were; inputs are never written."""

    def __init__(self, slots=None, joints: int = 17, channels: int = 2, score: bool = True, rate: float = 30.0, min_cutoff: float = 1.0, beta: float = 0.01,
                 d_cutoff: float = 1.0, min_score: float = 0.3, max_hold: int = 15, device=None, *, streams=None, track_slots=None, rows: str = "persons",
                 num_person: int = 1):
        who = "OneEuroFilter"
        (self.tracked, self.slots, self.joints, self.channels, self._Ct, self.streams, self.track_slots, self._rows_mode, self.R) = check_filter_args(
            slots, joints, channels, score, streams, track_slots, rows, num_person, who)
        self.score, self.rows = bool(score), (rows if self.tracked else None)
        self._params = one_euro_params(rate, min_cutoff, beta, d_cutoff, min_score, max_hold, who)
        self.device = _args.resolve_device((), device, who)
        self._lib = _lib.load()
        S, J, Cn = self.slots, self.joints, self.channels
        self._xhat = torch.zeros((S, J, Cn), dtype=torch.float32, device=self.device)
        self._dxhat = torch.zeros((S, J, Cn), dtype=torch.float32, device=self.device)
        self._last = torch.full((S, J), -1, dtype=torch.int64, device=self.device)
        self._owner = torch.zeros(S, dtype=torch.int32, device=self.device) if self.tracked else None
        self.tick = 0                                              # the tick of the next push with ticks=1

    def reset(self, slots=None, *, streams=None) -> None:
        """The slots (a filter built with ``slots=``; None: all) or every slot of the streams (a tracker-driven filter; None: all; what must accompany
        ``SortTracker.reset`` of the same streams) start again: their ``last`` entries become -1 and their owners 0.  ``xhat`` needs no clearing."""
        reset_filter(self, "OneEuroFilter.reset", slots, streams, "_last", -1)

    def push(self, x, track=None, *, slots=None, ticks: int = 1) -> torch.Tensor:
        """One tick.  A filter built with ``slots=``: ``x`` [slots,J,Ct] (every slot, in order) or, with ``slots=`` (distinct host integers), [K,J,Ct] for
        those slots.  A tracker-driven filter: ``x`` [B,R,J,Ct] or [B*R,J,Ct], row k of stream b as ``TrackedLifter.push`` takes it, and ``track``, this
        tick's ``TrackResult`` (read in place); a row the rule calls invalid is copied through.  float32, numpy or torch, on the host or on the filter's
        GPU.  ``ticks``: ticks since the previous push, above 1 after dropped frames.  Returns CUDA fp32 of ``x``'s shape; one launch."""
        xt, ids, fields, ticks = check_push(self, x, track, slots, ticks)
        J, lib, dev = self.joints, self._lib, self.device
        tick = self.tick + ticks - 1
        rows = xt.to(dev).contiguous()                             # a copy when it comes from the host; on the device the kernel only reads it
        out = torch.empty_like(rows)
        if self.tracked:
            t_ids, t_slot, t_born, t_count = (a.contiguous() for a in fields)
            with torch.cuda.device(dev):
                _lib.check(lib.kasf_one_euro_tracked(rows.data_ptr(), t_ids.data_ptr(), t_slot.data_ptr(), t_born.data_ptr(), t_count.data_ptr(), self.streams,
                                                     self.track_slots, self._rows_mode, self.R, J, self.channels, int(self.score), C.byref(self._params), tick,
                                                     self._xhat.data_ptr(), self._dxhat.data_ptr(), self._last.data_ptr(), self._owner.data_ptr(),
                                                     out.data_ptr(), None, _args.stream()))
        elif rows.shape[0] > 0:
            ids_d = torch.from_numpy(ids).to(dev) if ids is not None else None
            with torch.cuda.device(dev):
                _lib.check(lib.kasf_one_euro_push(rows.data_ptr(), ids_d.data_ptr() if ids_d is not None else None, int(rows.shape[0]), self.slots, J,
                                                  self.channels, int(self.score), C.byref(self._params), tick, self._xhat.data_ptr(), self._dxhat.data_ptr(),
                                                  self._last.data_ptr(), out.data_ptr(), _args.stream()))
        self.tick = tick + 1
        return out


def _track_rows(a, who: str) -> torch.Tensor:
    t = _args.as_tensor(a, who, "tracks", _args.FLOAT32)
    if t.dim() < 3:
        raise ValueError(f"{who}: expected tracks of [N,J,Ct], got {tuple(t.shape)}")
    return t


def smooth_tracks(tracks, offsets=None, *, score: bool = True, rate: float = 30.0, min_cutoff: float = 1.0, beta: float = 0.01, d_cutoff: float = 1.0,
                  min_score: float = 0.3, max_hold: int = 15, device=None):
    """Recorded tracks through the filter, each from an empty state with tick = frame index: what ``OneEuroFilter.push`` gives frame by frame, bit for bit, in
    one launch with the state in registers.  ``tracks``: a sequence of [N_i,J,Ct] float32 arrays (numpy or torch, on the host or the GPU, any N_i >= 0, never
    modified) -> a list of CUDA fp32 [N_i,J,Ct], views of one packed result; with ``offsets`` (integers [P+1] as ``lift_tracks`` takes them) one packed
    [sum N_i,J,Ct] array -> one packed tensor; one array [N,J,Ct] (a track) or [P,N,J,Ct] (P tracks of one length) -> its shape.  ``score``: the last of the
    Ct values is the score (keypoints; ``False`` for poses).  The parameters are ``OneEuroFilter``'s; the defaults are a starting point, not tuned."""
    who = "smooth_tracks"
    params = one_euro_params(rate, min_cutoff, beta, d_cutoff, min_score, max_hold, who)
    if not isinstance(score, (bool, np.bool_)):
        raise TypeError(f"{who}: score must be a bool, got {type(score).__name__}")
    parts, as_list = recorded_parts(tracks, offsets, who, lambda a: _track_rows(a, who), "J,Ct", True)
    if as_list and not parts:
        return []
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
    P, N = len(off) - 1, int(off[-1])
    if P > 0 and N > 0:
        off_d = torch.from_numpy(off).to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kasf_one_euro_tracks(packed.data_ptr(), off_d.data_ptr(), N, P, J, Cn, int(score), C.byref(params), out.data_ptr(), _args.stream()))
    return split(out, off) if as_list else out
