"""The seam between the tracker and the stream lifter, on the device: ``SortTracker``'s ids and slots drive per-player lifting histories without a read-back.

    trk = SortTracker(streams=B, slots=S_t, min_hits=0, num_person=P, hold_last=True)
    lifter = TrackedLifter(model, width, height, streams=B, track_slots=S_t, rows="persons", num_person=P,
                           flip=True, lag=0, layout="h36m")                  # width / height: one value or one per STREAM
    t = trk.update(d.boxes, d.count)
    r = crop_persons(frame, t.persons[0]); hm = pose_network(r.inputs)
    kp = heatmaps_to_keypoints(hm, r.center, r.scale, layout="h36m")          # [B*P,17,3] on the device
    out = lifter.push(kp, t)                   # or lifter.push_heatmaps(hm, r.center, r.scale, t)
    out.poses [B,R,17,3] fp32, out.valid [B,R] bool, out.ids [B,R] int32, out.frames [B,R] int64
    lifter.reset(streams=None)                 # goes with SortTracker.reset

``StreamLifter`` takes host integers for its slots, so a caller has to read ``t.ids`` / ``t.slot`` / ``t.count`` back every tick (a full synchronisation
with the forward in flight), decide births and deaths, and upload slot ids.  Here all of that is read from device memory inside two kernels
(``kasf_stream_track_front`` in front of the model's forward, ``kasf_stream_track_emit`` behind it); include/kasf.h states the rule:

* ``rows="persons"``: row k of stream b is the k-th oldest emitted track, the row order of ``t.persons`` (what the demo crops), track row
  ``r = count_b - 1 - k``; R = ``num_person``.  ``rows="tracks"``: row k is emitted row k of ``t.boxes``, ``r = k``; R = ``track_slots``.
* a row is valid iff ``k < min(count_b, R)``, ``id = t.ids[b,r] >= 1``, ``s = t.slot[b,r]`` in ``[0, track_slots)`` and no lower row of the stream has the
  same s.  Its history is slot ``g = b * track_slots + s``; when ``owner[g] != id`` or ``t.born[b,r] != 0`` the slot starts a new history for that id.  The
  frame is stored, and the row's pose is what ``StreamLifter`` gives for a slot with that history: ``lift_track`` of its last ``L = min(count, T)`` frames
  at the stream's resolution, frame ``max(L - 1 - lag, 0)``.
* a track that is not emitted gets no frame that tick and goes on when it comes back under the same id; a finished track's slot is left as it is.
* an invalid row touches no state; its pose is zero, ``valid`` 0, ``ids`` 0, ``frames`` 0.

``tail`` and ``replay`` are not offered: both need to know on the host which tracks ended.

On the device the rule is one function, ``csrc/tracked_rows.h``, which this lifter's kernel and the tracked kernels of ``OneEuroFilter`` and
``BoneLengthFilter`` all call; on the host the rows, streams and ``TrackResult`` arguments of all three are checked by ``_tracks.py``.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _args, _lib
from ._args import index_in
from .heatmap import check_decode_args, check_flip_args, check_heatmap_args
from .lift import _forward_windows, _model_device, _per_row, _upload
from .pose import check_layout, convert_frames
from .stream import _checked_tables, _decode_on
from ._tracks import ROWS, check_tracked_tick, fill_streams, float_rows, rows_mode, stream_ids, track_shape     # noqa: F401 -- ROWS and check_tracked_tick are offered here as before


class TrackedTick(NamedTuple):
    poses: torch.Tensor          # CUDA fp32 [B, R, 17, 3]: per row the pose `lag` frames behind its newest frame; zeros for an invalid row
    valid: torch.Tensor          # CUDA bool [B, R]
    ids: torch.Tensor            # CUDA int32 [B, R]: the track id of the row (TrackResult.ids), 0 for an invalid row
    frames: torch.Tensor         # CUDA int64 [B, R]: frames in the row's history after this push, 0 for an invalid row


def check_tracked_args(T, width, height, streams, track_slots, rows, num_person, lag, layout, who: str = "TrackedLifter"):
    """Everything the constructor can refuse without a device -> ``(T, width [B] float32, height [B] float32, streams, track_slots, rows mode, R, lag,
    whether the layout is COCO)``."""
    coco = check_layout(layout, who)
    mode = rows_mode(rows, who)
    T = int(T)
    if T < 1:
        raise ValueError(f"{who}: the model's n_frames must be >= 1, got {T}")
    streams, track_slots, R = track_shape(streams, track_slots, num_person, mode, who)
    lag = index_in(lag, who, "lag", 0, T - 1)
    w32, h32 = _per_row(width, streams, "width", who, "stream"), _per_row(height, streams, "height", who, "stream")
    return T, w32, h32, streams, track_slots, mode, R, lag, coco


def check_tracked_frames(kp: torch.Tensor, streams: int, R: int, who: str = "TrackedLifter.push"):
    """``keypoints`` [B,R,17,3] or [B*R,17,3] (already a float32 tensor) -> refuses any other shape."""
    if tuple(kp.shape) not in ((streams, R, 17, 3), (streams * R, 17, 3)):
        raise ValueError(f"{who}: expected keypoints [{streams},{R},17,3] or [{streams * R},17,3] (one frame per row), got {tuple(kp.shape)}")


class TrackedLifter:
    """Per-player lifting state of ``streams`` video streams on the model's device, driven by ``SortTracker.update``'s result; see the module docstring.

    All state is on the device and allocated once: ``ring [B*S_t,T,17,3]``, ``count [B*S_t]`` int64, ``owner [B*S_t]`` int32 (the track id whose history
    a slot holds), the resolutions and the two window tables.  There is no host copy of the counts and nothing in ``push`` synchronises with the host.
    ``layout="coco"``: the frames pushed are COCO-17 and go through ``coco_to_h36m``'s kernel first, one more launch per tick.

    Track ids restart at 1 after ``SortTracker.reset``, so a new player could be taken for the old owner of its slot: ``TrackedLifter.reset`` of the
    same streams must accompany every ``SortTracker.reset``.  ``tail`` and ``replay`` of ``StreamLifter`` are out of scope here (they need to know on
    the host which tracks ended).  Every refusal is raised before any launch and leaves the state as it was; inputs are never written."""

    def __init__(self, model, width, height, streams: int = 1, track_slots: int = 32, rows: str = "persons", num_person: int = 1, flip: bool = True,
                 lag: int = 0, layout: str = "h36m"):
        who = "TrackedLifter"
        self.device = _model_device(model, who)
        (self.T, w32, h32, self.streams, self.track_slots, self._rows_mode, self.R, self.lag, self._coco) = check_tracked_args(
            model.n_frames, width, height, streams, track_slots, rows, num_person, lag, layout, who)
        self.model, self.flip, self.rows, self.layout = model, bool(flip), rows, layout
        T, n = self.T, self.streams * self.track_slots
        self._lib = _lib.load()
        r_tab, fp_tab = _checked_tables(self._lib, T, who)
        self._r_tab, self._fp_tab, self._width, self._height = _upload(self.device, r_tab, fp_tab, w32, h32)
        self._ring = torch.zeros((n, T, 17, 3), dtype=torch.float32, device=self.device)
        self._count = torch.zeros(n, dtype=torch.int64, device=self.device)
        self._owner = torch.zeros(n, dtype=torch.int32, device=self.device)

    def reset(self, streams=None) -> None:
        """Zeroes count and owner of every slot of the given streams (an index or a sequence of indices; None: all of them): what must accompany
        ``SortTracker.reset`` of the same streams.  The ring needs no clearing: every position a window reads is written first."""
        idx = stream_ids(streams, self.streams, "TrackedLifter.reset")
        fill_streams(((self._count, 0), (self._owner, 0)), idx, self.streams, self.track_slots)

    def push(self, keypoints, track) -> TrackedTick:
        """One tick: ``keypoints`` [B,R,17,3] or [B*R,17,3] float32 pixel x, y, confidence -- row k of stream b belongs to the track the rule above names
        (with ``rows="persons"``: what ``crop_persons(frame, t.persons[b])`` and the pose network give) -- numpy or torch, on the host or, for a tick
        without any host synchronisation, on the model's GPU; ``track``: the ``TrackResult`` of this tick's ``SortTracker.update`` (or any object with
        CUDA int32 ``ids`` / ``slot`` / ``born`` [B,track_slots] and ``count`` [B]), read in place.  Returns ``TrackedTick``.  Two launches and one
        eval-mode forward of ``(1 + flip) * B * R`` clips, the same shape every tick."""
        who = "TrackedLifter.push"
        kp = float_rows(keypoints, self.device, who)
        check_tracked_frames(kp, self.streams, self.R, who)
        ids, slot, born, count_b = check_tracked_tick(track, self.streams, self.track_slots, self.device, who)
        B, R, T, n = self.streams, self.R, self.T, self.streams * self.R
        halves, lib, dev = (2 if self.flip else 1), self._lib, self.device
        frames = kp.to(dev).contiguous().view(n, 17, 3)            # a copy when it comes from the host; on the device the kernel only reads it
        ids, slot, born, count_b = ids.contiguous(), slot.contiguous(), born.contiguous(), count_b.contiguous()
        with torch.no_grad(), torch.cuda.device(dev):
            if self._coco:
                frames = convert_frames(frames)
            x = torch.empty((halves * n, T, 17, 3), dtype=torch.float32, device=dev)
            row_slot = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(lib.kasf_stream_track_front(frames.data_ptr(), ids.data_ptr(), slot.data_ptr(), born.data_ptr(), count_b.data_ptr(), B, self.track_slots,
                                                   self._rows_mode, R, T, self._ring.data_ptr(), self._count.data_ptr(), self._owner.data_ptr(),
                                                   self._width.data_ptr(), self._height.data_ptr(), self._r_tab.data_ptr(), int(self.flip), x.data_ptr(),
                                                   row_slot.data_ptr(), _args.stream()))
            pred = _forward_windows(self.model, x, n, halves, n)
            poses = torch.empty((B, R, 17, 3), dtype=torch.float32, device=dev)
            valid = torch.empty((B, R), dtype=torch.bool, device=dev)
            ids_out = torch.empty((B, R), dtype=torch.int32, device=dev)
            frames_out = torch.empty((B, R), dtype=torch.int64, device=dev)
            _lib.check(lib.kasf_stream_track_emit(pred.data_ptr(), int(self.flip), self._count.data_ptr(), self._owner.data_ptr(), row_slot.data_ptr(), n, T,
                                                  self._fp_tab.data_ptr(), self.lag, poses.data_ptr(), valid.data_ptr(), ids_out.data_ptr(),
                                                  frames_out.data_ptr(), _args.stream()))
        return TrackedTick(poses, valid, ids_out, frames_out)

    def push_heatmaps(self, heatmaps, center=None, scale=None, track=None, *, boxes=None, aspect=None, refine: bool = True, flipped=None,
                      shift: bool = True, pairs=None, decode: str = "quarter", kernel=None, sigma=None, udp=None) -> TrackedTick:
        """One tick straight from the pose network: ``heatmaps`` [B*R,17,H,W] or [B,R,17,H,W] (float32, float16 or bfloat16) with ``center`` / ``scale``
        or ``boxes`` and ``aspect`` as ``heatmaps_to_keypoints`` takes them, decoded on the device and pushed: what ``push`` returns for
        ``heatmaps_to_keypoints(..., layout="h36m")`` of them (for the COCO result on a ``layout="coco"`` lifter, which is the same frames).
        ``flipped`` / ``shift`` / ``pairs``: the flip test, and ``decode`` / ``kernel`` / ``sigma`` / ``udp``: the DARK / UDP sub-pixel decode, as
        ``heatmaps_to_keypoints`` takes them."""
        who = "TrackedLifter.push_heatmaps"
        hm, parts, kind, aspect = check_heatmap_args(heatmaps, center, scale, boxes, aspect, who)
        flip = check_flip_args(hm, flipped, shift, pairs, who)
        dark = check_decode_args(hm, decode, kernel, sigma, udp, refine, who)
        if tuple(hm.shape[:-3]) not in ((self.streams, self.R), (self.streams * self.R,)):
            raise ValueError(f"{who}: expected heatmaps [{self.streams * self.R},17,H,W] or [{self.streams},{self.R},17,H,W] (one person per row), "
                             f"got {tuple(hm.shape)}")
        if track is None:
            raise TypeError(f"{who}: track (the TrackResult of this tick) is required")
        check_tracked_tick(track, self.streams, self.track_slots, self.device, who)
        return self.push(_decode_on(self.device, hm, parts, kind, aspect, refine, not self._coco, who, flip, dark), track)
