"""Host-side handling of the track, slot and stream arguments that the lifters (lift.py, stream.py, tracked.py) and the filters (smooth.py, bones.py) share:
the one definition each of which rows a call takes, which slots or streams it names, which forms recorded tracks come in and how they are packed, and how a
filter's state starts again.  Like ``_args``, which it builds on: everything is refused or resolved without touching a device, except where a helper's
docstring says it moves or fills a tensor.  Every message begins with the caller's ``who`` and names the caller's own nouns, which are arguments here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in
from .track import MAX_PERSONS, MAX_SLOTS, MAX_STREAMS

ROWS = ("persons", "tracks")


def float_rows(a, device, who: str, name: str = "keypoints", owner: str = "the model") -> torch.Tensor:
    """float32 ``name`` as a tensor on the host or on ``device``, not moved (``_args.as_tensor``: a numpy array is shared, not copied); on another GPU than
    ``owner``'s they are refused."""
    t = _args.as_tensor(a, who, name, _args.FLOAT32)
    if t.is_cuda and t.device != device:
        raise RuntimeError(f"{who}: {name} are on {t.device}, {owner} on {device}")
    return t


def slot_ids(slots, S: int, who: str):
    """``slots=`` of a call -> distinct int32 ids [K] in [0, S) on the host (None: every slot in order)."""
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


def stream_ids(streams, B: int, who: str):
    """``streams=`` of a ``reset`` -> a list of stream indices in [0, B) (None: all of them)."""
    if streams is None:
        return None
    idx = np.atleast_1d(np.asarray(streams))
    if idx.dtype.kind not in "iu" or idx.ndim != 1:
        raise TypeError(f"{who}: streams must be an index or a sequence of indices, got {streams!r}")
    if idx.size and (idx.min() < 0 or idx.max() >= B):
        raise ValueError(f"{who}: streams must be in [0, {B}), got {idx.min()} .. {idx.max()}")
    return idx.tolist()


def rows_mode(rows, who: str) -> int:
    """``rows=`` of a tracker-driven object -> the KASF_ROWS_* constant."""
    if rows not in ROWS:
        raise ValueError(f"{who}: rows must be one of {ROWS}, got {rows!r}")
    return _lib.ROWS_PERSONS if rows == "persons" else _lib.ROWS_TRACKS


def track_shape(streams, track_slots, num_person, mode: int, who: str):
    """``streams`` / ``track_slots`` / ``num_person`` of a tracker-driven object, checked in that order -> ``(streams, track_slots, R)``, R the rows per stream."""
    streams = index_in(streams, who, "streams", 1, MAX_STREAMS)
    track_slots = index_in(track_slots, who, "track_slots", 1, MAX_SLOTS)
    num_person = index_in(num_person, who, "num_person", 1, MAX_PERSONS)
    return streams, track_slots, (num_person if mode == _lib.ROWS_PERSONS else track_slots)


def filter_slots(slots, streams, track_slots, rows, num_person, who: str):
    """How a filter is driven -> ``(tracked, S, streams, track_slots, rows mode, R)``: by host slot ids (``slots=``; the last four are None) or by a TrackResult
    (``streams=`` / ``track_slots=`` / ``rows=`` / ``num_person=``, S = streams * track_slots)."""
    tracked = streams is not None or track_slots is not None
    if tracked and slots is not None:
        raise ValueError(f"{who}: give slots= (host slot ids, as StreamLifter) or streams= and track_slots= (a TrackResult, as TrackedLifter), not both")
    if not tracked:
        if slots is None:
            raise ValueError(f"{who}: give slots= (host slot ids, as StreamLifter) or streams= and track_slots= (a TrackResult, as TrackedLifter)")
        return False, index_in(slots, who, "slots", 1, 2 ** 31 - 1), None, None, None, None
    mode = rows_mode(rows, who)
    streams, track_slots, R = track_shape(1 if streams is None else streams, 32 if track_slots is None else track_slots, num_person, mode, who)
    return True, streams * track_slots, streams, track_slots, mode, R


_TRACK_FIELDS = (("ids", 2), ("slot", 2), ("born", 2), ("count", 1))


def check_tracked_tick(track, streams: int, track_slots: int, device, who: str = "TrackedLifter.push"):
    """Everything ``push`` can refuse about a ``TrackResult`` without a device -> ``(ids, slot, born, count)``: int32 tensors [streams, track_slots] /
    [streams] on ``device``, taken as they are -- their contents are read by the kernel only, checking them here would synchronise."""
    out = []
    for name, dims in _TRACK_FIELDS:
        a = getattr(track, name, None)
        if not isinstance(a, torch.Tensor):
            raise TypeError(f"{who}: expected a TrackResult (SortTracker.update's), its {name} is {type(a).__name__}")
        if a.dtype != torch.int32:
            raise TypeError(f"{who}: TrackResult.{name} must be int32, got {a.dtype}")
        want = (streams, track_slots)[:dims]
        if tuple(a.shape) != want:
            raise ValueError(f"{who}: the lifter has {streams} streams of {track_slots} track slots, got TrackResult.{name} {tuple(a.shape)}")
        out.append(a.detach())
    for (name, _), a in zip(_TRACK_FIELDS, out):
        if a.device != device:
            raise RuntimeError(f"{who}: TrackResult.{name} is on {a.device}, the lifter on {device} (the tracker's output is read in place)")
    return tuple(out)


def check_push(f, x, track, slots, ticks, who: str = "OneEuroFilter.push"):
    """Everything a filter's ``push`` can refuse without a launch, for a filter (or any object) with ``tracked``, ``slots``, ``joints``, ``_Ct``, ``streams``,
    ``track_slots``, ``R`` and ``device`` -> ``(x as a float32 tensor where it is, host slot ids or None, the TrackResult's four tensors or None, ticks)``."""
    xt = float_rows(x, f.device, who, "rows", "the filter")
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
    ids = slot_ids(slots, f.slots, who)
    K = f.slots if ids is None else int(ids.size)
    if tuple(xt.shape) != (K, J, Ct):
        raise ValueError(f"{who}: expected rows [{K},{J},{Ct}] (one frame per pushed slot), got {tuple(xt.shape)}")
    return xt, ids, None, ticks


def fill_streams(states, idx, B: int, S_t: int) -> None:
    """``states``: (tensor [B * S_t, ...], value) pairs.  Fills every entry (``idx`` None) or, stream by stream, the entries of streams ``idx``, on the device."""
    views = [(t if idx is None else t.view(B, S_t, -1), v) for t, v in states]
    for b in [None] if idx is None else idx:
        for t, v in views:
            part = t if b is None else t[b]
            part.zero_() if v == 0 else part.fill_(v)


def reset_filter(f, who: str, slots, streams, state: str, value: int) -> None:
    """``reset`` of a filter whose per-slot tensor [S, ...] named ``state`` starts again at ``value``: by ``streams=`` for a tracker-driven one (its owners
    become 0 as well), by ``slots=`` otherwise.  The tensors are looked at only after everything is checked."""
    if f.tracked:
        if slots is not None:
            raise TypeError(f"{who}: a tracker-driven filter is reset by streams=, not by slots")
        idx = stream_ids(streams, f.streams, who)
        fill_streams(((getattr(f, state), value), (f._owner, 0)), idx, f.streams, f.track_slots)
        return
    if streams is not None:
        raise TypeError(f"{who}: a filter built with slots= is reset by slots, not by streams=")
    ids = slot_ids(slots, f.slots, who)
    if ids is None:
        fill_streams(((getattr(f, state), value),), None, 0, 0)
    elif ids.size:
        getattr(f, state).index_fill_(0, torch.from_numpy(ids.astype(np.int64)).to(f.device), value)


def recorded_parts(tracks, offsets, who: str, row, rows: str, four_forms: bool, exact: bool = False):
    """The forms recorded tracks come in -> ``(parts, as_list)``, the parts as ``row`` gives them, where they are.  Without ``offsets`` a sequence of [N_i, rows]
    arrays (with ``four_forms`` only a list or a tuple counts as one); with ``offsets`` one packed [sum N_i, rows] array; with ``four_forms`` also one track
    [N, rows] or [P, N, rows].  ``row(a)`` converts and checks one part; every part is converted before any is refused here for too many dimensions or, with
    ``exact``, for anything but three dimensions ending in (17, 3)."""
    as_list = offsets is None and (not four_forms or isinstance(tracks, (list, tuple)))
    parts = [row(a) for a in tracks] if as_list else [row(tracks)]
    most = 3 if as_list or offsets is not None else 4
    for a in parts:
        if a.dim() > most or (exact and (a.dim() != 3 or tuple(a.shape[1:]) != (17, 3))):
            form = f"tracks of [N,{rows}]" if as_list else f"packed tracks [sum N_i,{rows}]" if offsets is not None else f"[N,{rows}] or [P,N,{rows}]"
            raise ValueError(f"{who}: expected {form}, got {tuple(a.shape)}")
    return parts, as_list


def track_offsets(parts, offsets, as_list: bool, who: str) -> np.ndarray:
    """Where each track of ``recorded_parts``' parts begins -> int64 [P + 1] on the host: the caller's ``offsets``, checked against the packed length, or the
    running sum of a list's lengths, or P equal steps of N."""
    if offsets is not None:
        n = int(parts[0].shape[0])
        off = np.asarray(offsets.detach().cpu() if isinstance(offsets, torch.Tensor) else offsets)
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu" or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != n:
            raise ValueError(f"{who}: offsets must be integers [P+1] from 0 up to the packed length {n}, non-decreasing")
        return off.astype(np.int64)
    if as_list:
        return np.cumsum([0] + [a.shape[0] for a in parts], dtype=np.int64)
    lead = tuple(parts[0].shape[:-2])
    P, n = (1, lead[0]) if len(lead) == 1 else lead
    return np.arange(P + 1, dtype=np.int64) * n


def pack(parts, as_list: bool, dev) -> torch.Tensor:
    """The parts as one contiguous tensor on ``dev``: a list (not empty) packed on the host and uploaded once, or packed on the device if any part is already
    there; a single part moved as it is."""
    if as_list:
        return torch.cat([a.to(dev) for a in parts]) if any(a.is_cuda for a in parts) else torch.cat(parts).to(dev)
    return parts[0].to(dev).contiguous()


def split(out: torch.Tensor, off: np.ndarray):
    """A packed result as a list of views, one per track."""
    return [out[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
