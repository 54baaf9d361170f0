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
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in
from .tracked import ROWS, check_tracked_tick
from .track import MAX_PERSONS, MAX_SLOTS, MAX_STREAMS

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
    Ct = Cn + (1 if score else 0)
    tracked = streams is not None or track_slots is not None
    if tracked and slots is not None:
        raise ValueError(f"{who}: give slots= (host slot ids, as StreamLifter) or streams= and track_slots= (a TrackResult, as TrackedLifter), not both")
    if not tracked:
        if slots is None:
            raise ValueError(f"{who}: give slots= (host slot ids, as StreamLifter) or streams= and track_slots= (a TrackResult, as TrackedLifter)")
        S = index_in(slots, who, "slots", 1, 2 ** 31 - 1)
        return False, S, J, Cn, Ct, None, None, None, None
    if rows not in ROWS:
        raise ValueError(f"{who}: rows must be one of {ROWS}, got {rows!r}")
    streams = index_in(1 if streams is None else streams, who, "streams", 1, MAX_STREAMS)
    track_slots = index_in(32 if track_slots is None else track_slots, who, "track_slots", 1, MAX_SLOTS)
    num_person = index_in(num_person, who, "num_person", 1, MAX_PERSONS)
    R = num_person if rows == "persons" else track_slots
    return True, streams * track_slots, J, Cn, Ct, streams, track_slots, (_lib.ROWS_PERSONS if rows == "persons" else _lib.ROWS_TRACKS), R


def _rows_tensor(x, device, who: str) -> torch.Tensor:
    """float32 rows as a tensor on the host or on ``device``, not moved (``_args.as_tensor``; a tensor on another GPU is refused, as the lifters refuse it)."""
    t = _args.as_tensor(x, who, "rows", _args.FLOAT32)
    if t.is_cuda and t.device != device:
        raise RuntimeError(f"{who}: rows are on {t.device}, the filter on {device}")
    return t


def check_slot_ids(slots, S: int, who: str):
    """``slots=`` of a call -> distinct int32 ids [K] in [0, S) on the host (None: every slot in order), refused as ``StreamLifter`` refuses them."""
    if slots is None:
        return None
    if isinstance(slots, torch.Tensor):
        if slots.is_cuda:
            raise RuntimeError(f"{who}: slot ids are host integers, got a tensor on {slots.device}")
        slots = slots.numpy()
    ids = np.asarray(slots)
    if ids.size == 0:
        ids = ids.astype(np.int64)
    if ids.ndim != 1 or ids.dtype.kind not in "iu":
        raise ValueError(f"{who}: slots must be a 1-D sequence of integers, got shape {ids.shape} {ids.dtype}")
    if ids.size and (ids.min() < 0 or ids.max() >= S):
        raise ValueError(f"{who}: slot ids must be in [0, {S}), got {ids.tolist()}")
    if len(np.unique(ids)) != ids.size:
        raise ValueError(f"{who}: slot ids must be distinct, got {ids.tolist()}")
    return ids.astype(np.int32)


def check_stream_ids(streams, B: int, who: str):
    """``streams=`` of ``reset`` -> a list of stream indices (None: all of them), refused as ``TrackedLifter.reset`` refuses them."""
    if streams is None:
        return None
    idx = np.atleast_1d(np.asarray(streams))
    if idx.dtype.kind not in "iu" or idx.ndim != 1:
        raise TypeError(f"{who}: streams must be an index or a sequence of indices, got {streams!r}")
    if idx.size and (idx.min() < 0 or idx.max() >= B):
        raise ValueError(f"{who}: streams must be in [0, {B}), got {idx.min()} .. {idx.max()}")
    return idx.tolist()


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
        who = "OneEuroFilter.reset"
        if self.tracked:
            if slots is not None:
                raise TypeError(f"{who}: a tracker-driven filter is reset by streams=, not by slots")
            idx = check_stream_ids(streams, self.streams, who)
            if idx is None:
                self._last.fill_(-1)
                self._owner.zero_()
                return
            last, owner = self._last.view(self.streams, self.track_slots, self.joints), self._owner.view(self.streams, self.track_slots)
            for b in idx:
                last[b].fill_(-1)
                owner[b].zero_()
            return
        if streams is not None:
            raise TypeError(f"{who}: a filter built with slots= is reset by slots, not by streams=")
        ids = check_slot_ids(slots, self.slots, who)
        if ids is None:
            self._last.fill_(-1)
        elif ids.size:
            self._last.index_fill_(0, torch.from_numpy(ids.astype(np.int64)).to(self.device), -1)

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


def check_push(f, x, track, slots, ticks, who: str = "OneEuroFilter.push"):
    """Everything ``push`` can refuse without a launch, for a filter (or any object) with ``tracked``, ``slots``, ``joints``, ``_Ct``, ``streams``,
    ``track_slots``, ``R`` and ``device`` -> ``(x as a float32 tensor where it is, host slot ids or None, the TrackResult's four tensors or None, ticks)``."""
    xt = _rows_tensor(x, f.device, who)
    ticks = index_in(ticks, who, "ticks", 1, 2 ** 40)
    J, Ct = f.joints, f._Ct
    if f.tracked:
        if slots is not None:
            raise TypeError(f"{who}: a tracker-driven filter takes the tick's TrackResult, not slots=")
        B, R = f.streams, f.R
        if tuple(xt.shape) not in ((B, R, J, Ct), (B * R, J, Ct)):
            raise ValueError(f"{who}: expected rows [{B},{R},{J},{Ct}] or [{B * R},{J},{Ct}] (one frame per row), got {tuple(xt.shape)}")
        if track is None:
            raise TypeError(f"{who}: track (the TrackResult of this tick) is required")
        return xt, None, check_tracked_tick(track, B, f.track_slots, f.device, who), ticks
    if track is not None:
        raise TypeError(f"{who}: a filter built with slots= takes slots=, not a TrackResult")
    ids = check_slot_ids(slots, f.slots, who)
    K = f.slots if ids is None else int(ids.size)
    if tuple(xt.shape) != (K, J, Ct):
        raise ValueError(f"{who}: expected rows [{K},{J},{Ct}] (one frame per pushed slot), got {tuple(xt.shape)}")
    return xt, ids, None, ticks


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
    as_list = offsets is None and isinstance(tracks, (list, tuple))
    parts = [_track_rows(a, who) for a in tracks] if as_list else [_track_rows(tracks, who)]
    for a in parts:
        if a.dim() > (3 if as_list or offsets is not None else 4):
            raise ValueError(f"{who}: expected {'tracks of [N,J,Ct]' if as_list else 'packed tracks [sum N_i,J,Ct]' if offsets is not None else '[N,J,Ct] or [P,N,J,Ct]'}, "
                             f"got {tuple(a.shape)}")
    if as_list and not parts:
        return []
    J, Ct = int(parts[0].shape[-2]), int(parts[0].shape[-1])
    if any(tuple(a.shape[-2:]) != (J, Ct) for a in parts):
        raise ValueError(f"{who}: every track must have the same [J,Ct], got {[tuple(a.shape) for a in parts]}")
    Cn = Ct - (1 if score else 0)
    if not 1 <= J <= MAX_JOINTS or not 1 <= Cn <= MAX_CHANNELS:
        raise ValueError(f"{who}: need J in [1, {MAX_JOINTS}] and {'Ct - 1' if score else 'Ct'} in [1, {MAX_CHANNELS}], got rows [{J},{Ct}]")
    if offsets is not None:
        n = int(parts[0].shape[0])
        off = np.asarray(offsets.detach().cpu() if isinstance(offsets, torch.Tensor) else offsets)
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu" or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != n:
            raise ValueError(f"{who}: offsets must be integers [P+1] from 0 up to the packed length {n}, non-decreasing")
        off = off.astype(np.int64)
    elif as_list:
        off = np.cumsum([0] + [a.shape[0] for a in parts], dtype=np.int64)
    else:
        lead = tuple(parts[0].shape[:-2])
        P, n = (1, lead[0]) if len(lead) == 1 else lead
        off = np.arange(P + 1, dtype=np.int64) * n
    dev = _args.resolve_device(parts, device, who)
    if as_list:
        packed = torch.cat([a.to(dev) for a in parts]) if any(a.is_cuda for a in parts) else torch.cat(parts).to(dev)
    else:
        packed = parts[0].to(dev).contiguous()
    out = torch.empty_like(packed)
    P, N = len(off) - 1, int(off[-1])
    if P > 0 and N > 0:
        off_d = torch.from_numpy(off).to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kasf_one_euro_tracks(packed.data_ptr(), off_d.data_ptr(), N, P, J, Cn, int(score), C.byref(params), out.data_ptr(), _args.stream()))
    if as_list:
        return [out[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
    return out
