"""The step between the person detector and the crop: the demo's SORT tracker on the GPU the boxes were computed on.

    trk = SortTracker(streams=B, min_hits=0, num_person=2)               # the demo's Sort(min_hits=0), one tracker per video stream
    r = detections_to_boxes(prediction, width, height)                   # r.boxes [B,max_boxes,6], r.count [B]
    t = trk.update(r.boxes, r.count)                                      # one launch, no host synchronisation
    t.boxes [B,slots,4], t.ids, t.slot, t.born [B,slots], t.count, t.dropped [B], t.persons [B,num_person,4], t.person_count [B]
    crops = crop_persons(frame, t.persons[0])

``SortTracker.update`` is ``Sort.update`` (demo/lib/sort/sort.py:167-222: ``KalmanBoxTracker`` predict and update, ``iou``,
``associate_detections_to_trackers`` with scipy's ``linear_sum_assignment``, births, deaths, the output newest first) and, from ``gen_video_kpts``
(demo/lib/hrnet/gen_kpts.py:125-143), the empty-frame hold and the ``num_person`` oldest tracks -- one launch per tick for all streams, the same bits from
run to run.  The Kalman filter runs in fp64 as the reference's does.  filterpy is not installed where this was written: its ``KalmanFilter.update`` is
restated from its published form, not recorded.  include/kasf.h (``kasf_sort_update``) states every rule.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import _args, _lib
from ._args import index_in

MAX_SLOTS = MAX_DETS = _lib.SORT_MAX        # a track and a detection each take one lane of a wavefront
MAX_STREAMS, MAX_PERSONS = 65535, 65535


class TrackResult(NamedTuple):
    boxes: torch.Tensor          # CUDA fp32 [B, slots, 4]: x1, y1, x2, y2 of the emitted tracks, newest track first (what crop_persons takes); rows past count are 0
    ids: torch.Tensor            # CUDA int32 [B, slots]: the reference's id + 1 (ids start at 1 in every stream); -1 past count
    slot: torch.Tensor           # CUDA int32 [B, slots]: the track's slot in [0, slots), its own from birth to death
    born: torch.Tensor           # CUDA int32 [B, slots]: 1 on the tick the track was founded
    count: torch.Tensor          # CUDA int32 [B]: rows emitted
    dropped: torch.Tensor        # CUDA int32 [B]: births dropped this tick because all slots were taken
    persons: torch.Tensor        # CUDA fp32 [B, num_person, 4]: the k-th OLDEST emitted track (the demo's people_track[-num_person:][::-1]); rows past person_count are 0
    person_count: torch.Tensor   # CUDA int32 [B]: min(count, num_person)


class TrackState(NamedTuple):
    x: torch.Tensor              # CUDA fp64 [B, slots, 7] per list position: cx, cy, s, r, vx, vy, vs
    P: torch.Tensor              # CUDA fp64 [B, slots, 7, 7]
    boxes: torch.Tensor          # CUDA fp64 [B, slots, 4]: the box of x
    ids: torch.Tensor            # CUDA int32 [B, slots]: the reference's id (0-based), and below its other counters
    slot: torch.Tensor
    time_since_update: torch.Tensor
    hits: torch.Tensor
    hit_streak: torch.Tensor
    age: torch.Tensor
    tracks: torch.Tensor         # CUDA int32 [B]: list length; positions past it are 0
    next_id: torch.Tensor        # CUDA int32 [B]
    ticks: torch.Tensor          # CUDA int32 [B]: the reference's frame_count


def check_tracker_args(streams, slots, max_age, min_hits, iou_threshold, num_person, who: str = "SortTracker"):
    """Everything the constructor can refuse without a device."""
    streams = index_in(streams, who, "streams", 1, MAX_STREAMS)
    slots = index_in(slots, who, "slots", 1, MAX_SLOTS)
    max_age = index_in(max_age, who, "max_age", 0, 2 ** 31 - 1)
    min_hits = index_in(min_hits, who, "min_hits", 0, 2 ** 31 - 1)
    num_person = index_in(num_person, who, "num_person", 1, MAX_PERSONS)
    try:
        iou_threshold = float(iou_threshold)
    except (TypeError, ValueError):
        raise TypeError(f"{who}: iou_threshold must be a number, got {type(iou_threshold).__name__}") from None
    if not math.isfinite(iou_threshold):
        raise ValueError(f"{who}: iou_threshold must be finite, got {iou_threshold!r}")
    return streams, slots, max_age, min_hits, iou_threshold, num_person


def check_update_args(boxes, count, streams: int, who: str = "SortTracker.update"):
    """Everything ``update`` can refuse without a device -> ``(boxes [B,n,>=4] float32 tensor where it is, count [B] int32 tensor or None)``."""
    t = _args.as_tensor(boxes, who, "boxes", _args.FLOAT32)
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[2] < 4:
        raise ValueError(f"{who}: expected boxes [B,n,>=4] or [n,>=4] = x1, y1, x2, y2, ..., got {tuple(boxes.shape)}")
    if t.shape[0] != streams:
        raise ValueError(f"{who}: the tracker has {streams} streams, got boxes for {t.shape[0]}")
    if t.shape[1] > MAX_DETS:
        raise ValueError(f"{who}: at most {MAX_DETS} detections per stream, got {t.shape[1]}")
    if count is None:
        return t, None
    if isinstance(count, torch.Tensor) and count.is_cuda:          # taken as it is: checking it would synchronise
        if count.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{who}: count must be int32 or int64, got {count.dtype}")
        c = count.detach().to(torch.int32)
    else:
        v = np.asarray(count.detach() if isinstance(count, torch.Tensor) else count)
        if v.dtype.kind not in "iu":
            raise TypeError(f"{who}: count must be integers, got {v.dtype}")
        if v.size and (v.min() < 0 or v.max() > t.shape[1]):
            raise ValueError(f"{who}: count must be in [0, {t.shape[1]}], got {v.min()} .. {v.max()}")
        c = torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32))
    if c.dim() == 0:
        c = c[None]
    if tuple(c.shape) != (streams,):
        raise ValueError(f"{who}: expected count [{streams}], got {tuple(c.shape)}")
    return t, c


class SortTracker:
    """The reference's ``Sort`` for ``streams`` independent video streams, on the GPU.  The defaults are the reference class's (``max_age=1, min_hits=3``,
    ``iou_threshold=0.3``); the demo constructs ``Sort(min_hits=0)`` and follows ``num_person`` people (gen_kpts.py:111).

    ``slots``: the most tracks a stream holds, at most 64; a birth beyond it is dropped and counted in ``dropped``.  Every track keeps one ``slot`` in
    [0, slots) from birth to death.  ``num_person``: rows of ``persons``, the oldest emitted tracks first.  ``hold_last``: a tick without a valid
    detection runs on the stream's last non-empty detections, as ``gen_video_kpts`` does with ``bboxs_pre``.  ``device``: the GPU the state lives on
    (default: the current one).

    Deliberately unlike the reference: ids count per stream, from 1 (the reference's counter is shared by every ``Sort`` of the process); a track whose
    predicted box is not finite is dropped; a detection with a non-finite coordinate or ``y2 <= y1`` is ignored; between assignments of exactly equal
    total IoU the choice need not be scipy's; the host-side ``round(i, 2)`` is not applied.  There is no host path: without a GPU the constructor raises
    ``RuntimeError``.  Every refusal comes before any launch."""

    def __init__(self, streams: int = 1, slots: int = 32, max_age: int = 1, min_hits: int = 3, iou_threshold: float = 0.3, num_person: int = 1,
                 hold_last: bool = False, device=None):
        who = "SortTracker"
        (self.streams, self.slots, self.max_age, self.min_hits, self.iou_threshold, self.num_person) = check_tracker_args(
            streams, slots, max_age, min_hits, iou_threshold, num_person, who)
        self.hold_last = bool(hold_last)
        self.device = dev = _args.resolve_device((), device, who)
        nbytes = _lib.load().kasf_sort_state_bytes(self.streams, self.slots, MAX_DETS)
        if nbytes < 0:
            _lib.check(2)
        self._stride = nbytes // self.streams
        self._state = torch.zeros((self.streams, self._stride), dtype=torch.uint8, device=dev)       # all zero = an empty tracker

    def reset(self, streams=None) -> None:
        """Empties every stream, or the given ones (an index or a sequence of indices): their tracks, id counter, tick count and held detections."""
        if streams is None:
            self._state.zero_()
            return
        idx = np.atleast_1d(np.asarray(streams))
        if idx.dtype.kind not in "iu" or idx.ndim != 1:
            raise TypeError(f"SortTracker.reset: streams must be an index or a sequence of indices, got {streams!r}")
        if idx.size and (idx.min() < 0 or idx.max() >= self.streams):
            raise ValueError(f"SortTracker.reset: streams must be in [0, {self.streams}), got {idx.min()} .. {idx.max()}")
        for b in idx.tolist():
            self._state[b].zero_()

    def update(self, boxes, count=None) -> TrackResult:
        """One tick for every stream.  ``boxes`` [B,n,>=4] (or [n,>=4] with one stream) float32 = x1, y1, x2, y2 in the first four columns, n <= 64:
        ``DetectResult.boxes`` as it is -- a GPU tensor is read in place, also a strided view as long as its columns are adjacent (any other view is packed
        first); numpy / torch on the host is uploaded.  ``count`` [B]: the rows that count (``DetectResult.count``; a GPU tensor is taken as it is and
        clamped to [0, n] in the kernel); None = all n.  A stream without detections still has to be ticked, with count 0.

        Returns ``TrackResult``; ``t.boxes[b, :t.count[b]]`` are the tracks ``Sort.update`` returns, newest first, ``t.ids`` their last column.  Nothing in
        the call synchronises with the host."""
        who = "SortTracker.update"
        t, c = check_update_args(boxes, count, self.streams, who)
        for a in (t, c):
            if a is not None and a.is_cuda and a.device != self.device:
                raise RuntimeError(f"{who}: input on {a.device}, the tracker is on {self.device}")
        t = t.to(self.device)
        if t.stride(2) != 1 or t.stride(1) < 4 or t.stride(0) < 0:
            t = t.contiguous()
        c = None if c is None else c.to(self.device).contiguous()
        B, S, NP = self.streams, self.slots, self.num_person
        dev = self.device
        out_boxes = torch.empty((B, S, 4), dtype=torch.float32, device=dev)
        ints = torch.empty((3, B, S), dtype=torch.int32, device=dev)
        per = torch.empty((3, B), dtype=torch.int32, device=dev)
        persons = torch.empty((B, NP, 4), dtype=torch.float32, device=dev)
        n = int(t.shape[1])
        with torch.cuda.device(dev):
            _lib.check(_lib.load().kasf_sort_update(
                self._state.data_ptr(), B, S, MAX_DETS, t.data_ptr() if n else None, n, int(t.stride(0)) if n else 0, int(t.stride(1)) if n else 4,
                None if c is None else c.data_ptr(), self.max_age, self.min_hits, self.iou_threshold, NP, int(self.hold_last), out_boxes.data_ptr(),
                ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), per[0].data_ptr(), per[1].data_ptr(), persons.data_ptr(), per[2].data_ptr(),
                _args.stream()))
        return TrackResult(out_boxes, ints[0], ints[1], ints[2], per[0], per[1], persons, per[2])

    def state(self) -> TrackState:
        """The trackers as they stand, per list position (oldest track first), as copies: the fp64 Kalman state ``x`` and covariance ``P`` (dense [7,7]; the
        kernel keeps its four blocks, every other entry is 0), the box of ``x`` and the reference's counters.  For tests and inspection."""
        B, S = self.streams, self.slots
        st = self._state
        hdr = st[:, :_lib.SORT_HEADER_BYTES].contiguous().view(torch.int32)
        o = _lib.SORT_HEADER_BYTES
        x = st[:, o:o + 56 * S].contiguous().view(torch.float64).view(B, 7, S).transpose(1, 2).contiguous()
        o += 56 * S
        blk = st[:, o:o + 104 * S].contiguous().view(torch.float64).view(B, 13, S)
        o += 104 * S
        ints = st[:, o:o + 24 * S].contiguous().view(torch.int32).view(B, 6, S)
        P = torch.zeros((B, S, 7, 7), dtype=torch.float64, device=st.device)
        for k in range(3):
            P[:, :, k, k], P[:, :, k, k + 4], P[:, :, k + 4, k], P[:, :, k + 4, k + 4] = blk[:, 4 * k], blk[:, 4 * k + 1], blk[:, 4 * k + 2], blk[:, 4 * k + 3]
        P[:, :, 3, 3] = blk[:, 12]
        w = torch.sqrt(x[..., 2] * x[..., 3])
        h = x[..., 2] / w
        boxes = torch.stack((x[..., 0] - w / 2.0, x[..., 1] - h / 2.0, x[..., 0] + w / 2.0, x[..., 1] + h / 2.0), dim=-1)
        live = torch.arange(S, device=st.device)[None, :] < hdr[:, 0:1]
        boxes = torch.where(live[..., None], boxes, torch.zeros_like(boxes))
        return TrackState(x, P, boxes, *(ints[:, k].clone() for k in range(6)), hdr[:, 0].clone(), hdr[:, 1].clone(), hdr[:, 2].clone())
