"""Constant limb lengths per player, on the device: one length per bone per track, re-imposed on every frame.

    poses = fix_bone_lengths(poses)                            # [N,17,3] -> the same shape, CUDA fp32; the track's own medians
    poses = fix_bone_lengths(packed, offsets=offsets)          # recorded tracks as smooth_tracks takes them: also a list of [N_i,17,3] or [P,N,17,3]
    poses = fix_bone_lengths(poses, lengths=athlete16)         # a measured table [16] (or [P,16]) instead of the medians
    lengths, counts = bone_lengths(packed, offsets)            # [P,16] fp32 medians, [P,16] int32 usable samples
    fb = BoneLengthFilter(slots=32, window=64)                 # live: a running mean per slot; BoneLengthFilter(streams=B, track_slots=S_t, ...) reads a TrackResult
    poses = fb.push(f3.push(out.poses, t), t)                  # behind the lifter and the One-Euro filter over its poses

The lift predicts every window on its own and the One-Euro filter steadies positions, not the skeleton, so a thigh still breathes by a few percent from frame
to frame.  include/kasf.h (``kasf_bone_median``) states the rule in full: bone k joins joint k + 1 to its parent in the model's own table
(``draw.H36M_SEGMENTS``); a track's target length of a bone is the lower median of its lengths over the usable (all-finite) frames; every usable frame is then
walked from the root, each bone scaled to its target, so directions, joint angles and the root stay as they were.  ``symmetric`` gives the left / right partner
bones their mean.  A length of 0 in a table means "leave this bone alone"; a frame with a NaN or an infinity is copied through.

Everything runs on the device and nothing is read back: two launches for the medians (lengths, then a radix select per track and bone), one for the walk, one
per ``push``.  There is no host path.  The live form is a running mean over the first ``window`` frames and an exponential average after them, not a median,
and ``window`` is a starting point, not tuned on footage.

The tracker-driven filter resolves its rows by ``TrackedLifter``'s rule, one device function (``csrc/tracked_rows.h``); its slot, stream and recorded-track
arguments go through ``_tracks.py``, as ``OneEuroFilter``'s and the lifters' do.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in
from ._tracks import check_push, filter_slots, pack, recorded_parts, reset_filter, split, track_offsets

BONES, MAX_WINDOW = 16, 1 << 20
BONE_PARENTS = (0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)       # bone k joins joint k + 1 to BONE_PARENTS[k]
BONE_PARTNERS = ((0, 3), (1, 4), (2, 5), (10, 13), (11, 14), (12, 15))     # left / right, from joint_flip's lists


def _pose_rows(a, who: str) -> torch.Tensor:
    t = _args.as_tensor(a, who, "poses", _args.FLOAT32)
    if t.dim() < 3 or tuple(t.shape[-2:]) != (17, 3):
        raise ValueError(f"{who}: expected poses of [N,17,3], got {tuple(t.shape)}")
    return t


def _bool(v, who: str, name: str) -> bool:
    if not isinstance(v, (bool, np.bool_)):
        raise TypeError(f"{who}: {name} must be a bool, got {type(v).__name__}")
    return bool(v)


def _tracks(poses, offsets, who: str):
    """The four input forms (``_tracks.recorded_parts``) -> (the parts where they are, offsets int64 [P+1] on the host, as_list); everything that can be
    refused without a device is refused here, before the device is resolved."""
    parts, as_list = recorded_parts(poses, offsets, who, lambda a: _pose_rows(a, who), "17,3", True)
    off = track_offsets(parts, offsets, as_list, who)
    if int(off[-1]) >= 2 ** 31:
        raise ValueError(f"{who}: at most 2^31 - 1 frames in a call, got {int(off[-1])}")
    return parts, off, as_list


def _packed(parts, as_list, dev) -> torch.Tensor:
    if as_list and not parts:
        return torch.empty((0, 17, 3), dtype=torch.float32, device=dev)
    return pack(parts, as_list, dev).view(-1, 17, 3)


def _medians(lib, packed, off_d, N: int, P: int, dev, want_counts: bool):
    lengths = torch.empty((P, BONES), dtype=torch.float32, device=dev)
    counts = torch.empty((P, BONES), dtype=torch.int32, device=dev) if want_counts else None
    if P > 0:
        scratch = torch.empty(max(N, 1) * BONES, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.kasf_bone_median(packed.data_ptr(), off_d.data_ptr(), N, P, scratch.data_ptr(), lengths.data_ptr(),
                                            counts.data_ptr() if want_counts else None, _args.stream()))
    return lengths, counts


def bone_lengths(poses, offsets=None, *, device=None):
    """The target lengths of recorded tracks: ``poses`` in one of ``fix_bone_lengths``' four forms -> ``(lengths [P,16] float32, counts [P,16] int32)`` on the
    device: per track and bone the lower median of the usable lengths and how many there were (0 and 0 for a bone that never had one).  Two launches."""
    who = "bone_lengths"
    parts, off, as_list = _tracks(poses, offsets, who)
    dev = _args.resolve_device(parts, device, who)
    lib = _lib.load()
    packed = _packed(parts, as_list, dev)
    P, N = len(off) - 1, int(off[-1])
    return _medians(lib, packed, torch.from_numpy(off).to(dev), N, P, dev, True)


def fix_bone_lengths(poses, offsets=None, *, lengths=None, symmetric: bool = False, return_lengths: bool = False, device=None):
    """Recorded tracks with every bone at one length per track.  ``poses``: a sequence of [N_i,17,3] float32 arrays (numpy or torch, on the host or the GPU,
    any N_i >= 0, never modified) -> a list of CUDA fp32 [N_i,17,3], views of one packed result; with ``offsets`` (integers [P+1]) one packed [sum N_i,17,3]
    array -> one packed tensor; one array [N,17,3] (a track) or [P,N,17,3] (P tracks of one length) -> its shape.  ``lengths``: None for each track's own
    medians (``bone_lengths``), or a float32 table [16] for every track or [P,16], e.g. a measured athlete; 0 leaves a bone alone.  ``symmetric``: left / right
    partner bones get their mean before use.  ``return_lengths``: also return the table as given or found, before ``symmetric``, on the device.  At most three
    launches, nothing read back."""
    who = "fix_bone_lengths"
    parts, off, as_list = _tracks(poses, offsets, who)
    symmetric, return_lengths = _bool(symmetric, who, "symmetric"), _bool(return_lengths, who, "return_lengths")
    P, N = len(off) - 1, int(off[-1])
    if as_list and not parts and lengths is None and not return_lengths:
        return []
    table = None
    if lengths is not None:
        table = _args.as_tensor(lengths, who, "lengths", _args.FLOAT32)
        if tuple(table.shape) not in ((BONES,), (P, BONES)):
            raise ValueError(f"{who}: lengths must be [{BONES}] or [{P},{BONES}] float32, got {tuple(table.shape)}")
    dev = _args.resolve_device(parts + ([table] if table is not None else []), device, who)
    lib = _lib.load()
    packed = _packed(parts, as_list, dev)
    off_d = torch.from_numpy(off).to(dev)
    if table is None:
        table, _ = _medians(lib, packed, off_d, N, P, dev, False)
    else:
        table = table.to(dev).contiguous()
    out = torch.empty_like(packed)
    if N > 0:
        with torch.cuda.device(dev):
            _lib.check(lib.kasf_bone_apply(packed.data_ptr(), off_d.data_ptr(), N, P, table.data_ptr(), int(table.dim() == 2), int(symmetric), out.data_ptr(),
                                           _args.stream()))
    result = split(out, off) if as_list else out.view(parts[0].shape)
    return (result, table) if return_lengths else result


class BoneLengthFilter:
    """Constant limb lengths over the rows of a live pipeline, the state (``len``, ``cnt`` [S,16], ``owner`` [S]) on the device; see the module docstring and
    include/kasf.h (``kasf_bone_push``).  Built with ``slots=`` it is driven by host slot ids like ``StreamLifter``; built with ``streams=`` / ``track_slots=``
    / ``rows=`` / ``num_person=`` (``TrackedLifter``'s words) it reads the slot, the births and the deaths of every row from this tick's ``TrackResult`` on the
    device by ``OneEuroFilter``'s rule, so the two agree on whose history a row continues.  A slot's table is the running mean of each bone over its first
    ``window`` frames and an exponential average of weight 1 / ``window`` after them: a mean, not a median, and the default ``window`` is a starting point,
    not tuned on footage.  Every refusal is raised before any launch and leaves the state as it was; inputs are never written."""

    joints, channels, score, _Ct = 17, 3, False, 3

    def __init__(self, slots=None, window: int = 64, symmetric: bool = False, device=None, *, streams=None, track_slots=None, rows: str = "persons",
                 num_person: int = 1):
        who = "BoneLengthFilter"
        self.tracked, self.slots, self.streams, self.track_slots, self._rows_mode, self.R = filter_slots(slots, streams, track_slots, rows, num_person, who)
        self.rows = rows if self.tracked else None
        self.window = index_in(window, who, "window", 1, MAX_WINDOW)
        self.symmetric = _bool(symmetric, who, "symmetric")
        self.device = _args.resolve_device((), device, who)
        self._lib = _lib.load()
        self._len = torch.zeros((self.slots, BONES), dtype=torch.float32, device=self.device)
        self._cnt = torch.zeros((self.slots, BONES), dtype=torch.int32, device=self.device)
        self._owner = torch.zeros(self.slots, dtype=torch.int32, device=self.device) if self.tracked else None

    def reset(self, slots=None, *, streams=None) -> None:
        """The slots (a filter built with ``slots=``; None: all) or every slot of the streams (a tracker-driven filter; None: all; what must accompany
        ``SortTracker.reset`` of the same streams) start again: their counts, and their owners, become 0."""
        reset_filter(self, "BoneLengthFilter.reset", slots, streams, "_cnt", 0)

    def push(self, poses, track=None, *, slots=None) -> torch.Tensor:
        """One tick.  A filter built with ``slots=``: ``poses`` [slots,17,3] (every slot, in order) or, with ``slots=`` (distinct host integers), [K,17,3] for
        those slots.  A tracker-driven filter: ``poses`` [B,R,17,3] or [B*R,17,3], row k of stream b as ``TrackedLifter.push`` takes it, and ``track``, this
        tick's ``TrackResult`` (read in place); a row the rule calls invalid is copied through.  float32, numpy or torch, on the host or on the filter's GPU.
        Returns CUDA fp32 of ``poses``' shape; one launch."""
        xt, ids, fields, _ = check_push(self, poses, track, slots, 1, "BoneLengthFilter.push")
        lib, dev = self._lib, self.device
        rows = xt.to(dev).contiguous()
        out = torch.empty_like(rows)
        if self.tracked:
            t_ids, t_slot, t_born, t_count = (a.contiguous() for a in fields)
            with torch.cuda.device(dev):
                _lib.check(lib.kasf_bone_tracked(rows.data_ptr(), t_ids.data_ptr(), t_slot.data_ptr(), t_born.data_ptr(), t_count.data_ptr(), self.streams,
                                                 self.track_slots, self._rows_mode, self.R, self.window, int(self.symmetric), self._len.data_ptr(),
                                                 self._cnt.data_ptr(), self._owner.data_ptr(), out.data_ptr(), None, _args.stream()))
        elif rows.shape[0] > 0:
            ids_d = torch.from_numpy(ids).to(dev) if ids is not None else None
            with torch.cuda.device(dev):
                _lib.check(lib.kasf_bone_push(rows.data_ptr(), ids_d.data_ptr() if ids_d is not None else None, int(rows.shape[0]), self.slots, self.window,
                                              int(self.symmetric), self._len.data_ptr(), self._cnt.data_ptr(), out.data_ptr(), _args.stream()))
        return out
