"""Lifting live keypoint streams frame by frame: the online form of ``lift_track`` / ``lift_tracks`` (demo/demo.py:194-254, ``lift_3d_pose``).

    lifter = StreamLifter(model, width, height, slots=32, flip=True, lag=0)      # width / height: one value or one per slot; layout="coco": COCO-17 frames in
    poses = lifter.push(kp)                     # kp [slots,17,3] fp32 pixels + confidence, one new frame for every slot -> CUDA fp32 [slots,17,3]
    poses = lifter.push(kp, slots=[3, 7, 8])    # kp [3,17,3]: only these slots got a frame this tick -> [3,17,3]
    poses = lifter.push_heatmaps(hm, center, scale)    # hm [slots,17,H,W]: the pose network's output, decoded on the device, then pushed
    rest = lifter.tail(slots=[3])               # [1,lag,17,3]: the frames push has not emitted yet, at the end of a track
    lifter.reset(slots=[7])                     # the player left: the slot starts a new history
    poses = lifter.replay(track)                # a recorded [N,17,3] / [P,N,17,3] track tick by tick, through a temporary state

A *slot* holds one player's recent frames on the device (``ring [slots,T,17,3]``, ``count [slots]``).  With k frames since its reset, the slot's current
window is its last L = min(k, T) frames, and the poses of that window are ``lift_track(model, window, width, height, flip=flip)``: during warm-up (k < T)
the demo's one resampled clip of a track shorter than T (``turn_into_clips``, demo.py:138-156), afterwards the sliding window of the last T frames.
``push`` returns frame ``max(L - 1 - lag, 0)`` of it (``lag`` = frames of look-ahead the caller waits for; 0: the newest frame), ``tail`` the ``lag`` frames
after that one.  A tick is one upload of the new frames, three launches (``kasf_stream_push`` / ``_windows`` / ``_emit``) and one eval-mode forward of
``(1 + flip) * K`` clips; nothing is planned, tabulated or read back per tick.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _args, _lib
from .heatmap import check_decode_args, check_flip_args, check_heatmap_args, decode
from .pose import check_layout, convert_frames
from .lift import _forward_windows, _model_device, _per_row, _upload, window_plan
from ._tracks import float_rows, slot_ids


def stream_tables(T: int):
    """``(resample_tab, first_pos_tab)``, int32 [T+1, T]: row n (1 <= n < T) holds ``window_plan(n, T)``'s ``resample`` and ``first_pos`` (the latter in
    its first n entries, zeros after), row T the identity 0 .. T-1 in both, row 0 zeros -- what ``kasf_stream_tables`` builds in C."""
    T = int(T)
    if T < 1:
        raise ValueError(f"stream_tables: T must be >= 1, got {T}")
    resample, first_pos = np.zeros((T + 1, T), np.int32), np.zeros((T + 1, T), np.int32)
    for n in range(1, T):
        _, _, r, fp = window_plan(n, T)
        resample[n], first_pos[n, :n] = r, fp
    resample[T] = first_pos[T] = np.arange(T, dtype=np.int32)
    return resample, first_pos


def _checked_tables(lib, T: int, who: str):
    """``stream_tables(T)``, held to what the library's ``kasf_stream_tables`` builds."""
    r_tab, fp_tab = stream_tables(T)
    c_r, c_fp = np.full_like(r_tab, -1), np.full_like(fp_tab, -1)
    if lib.kasf_stream_tables(T, c_r.ctypes.data, c_fp.ctypes.data) != 0 or not np.array_equal(c_r, r_tab) or not np.array_equal(c_fp, fp_tab):
        raise _lib.KasfError(f"{who}: the library's window tables disagree with stream_tables (stale build?)")
    return r_tab, fp_tab


def _decode_on(device, hm, parts, kind, aspect, refine: bool, h36m: bool, who: str, flip=None, dark=None) -> torch.Tensor:
    """``push_heatmaps``: the checked heatmaps and their geometry (and ``check_flip_args``' and ``check_decode_args``' results), refused when on another GPU,
    decoded on ``device`` -> keypoints [n,17,3]."""
    for t in (hm,) + parts + ((flip[0],) if flip is not None else ()):
        if t.is_cuda and t.device != device:
            raise RuntimeError(f"{who}: input on {t.device}, the model on {device}")
    if flip is not None:
        flip = (flip[0].to(device),) + flip[1:]
    return decode(hm.to(device), tuple(t.to(device) for t in parts), kind, aspect, refine, h36m, flip, dark=dark)


class StreamLifter:
    """Per-player lifting state on the model's device; see the module docstring.  ``counts`` (host int64 [slots]) mirrors the device's frame counts and is
    what validates calls: every refusal is raised before any kernel runs and leaves the state as it was.  Inputs are never modified.
    ``layout="coco"``: every frame pushed (``replay``'s tracks included) is COCO-17 pixel x, y, score and goes through ``coco_to_h36m`` on the device
    before it is stored, one more launch per tick: the ring holds H36M frames, and the window and emit kernels see nothing new."""

    def __init__(self, model, width, height, slots: int = 32, flip: bool = True, lag: int = 0, layout: str = "h36m", _tables=None):
        self.layout, self._coco = layout, check_layout(layout, "StreamLifter")
        self.device = _model_device(model, "StreamLifter")
        self.model, self.flip = model, bool(flip)
        self.T = T = int(model.n_frames)
        self.slots = S = int(slots)
        if S < 1:
            raise ValueError(f"StreamLifter: slots must be >= 1, got {slots}")
        self.lag = int(lag)
        if not 0 <= self.lag <= T - 1:
            raise ValueError(f"StreamLifter: lag must be in [0, T - 1 = {T - 1}], got {lag}")
        w32, h32 = _per_row(width, S, "width", "StreamLifter", "slot"), _per_row(height, S, "height", "StreamLifter", "slot")
        one = all((v.dim() if isinstance(v, torch.Tensor) else np.ndim(v)) == 0 for v in (width, height))
        self._one_resolution = (float(w32[0]), float(h32[0])) if one else None      # what replay lifts a recorded track at
        self._lib = _lib.load()
        self._tables = _tables = _checked_tables(self._lib, T, "StreamLifter") if _tables is None else _tables
        self._r_tab, self._fp_tab, self._width, self._height = _upload(self.device, _tables[0], _tables[1], w32, h32)
        self._ring = torch.zeros((S, T, 17, 3), dtype=torch.float32, device=self.device)
        self._count = torch.zeros(S, dtype=torch.int64, device=self.device)
        self._counts = np.zeros(S, np.int64)

    @property
    def counts(self) -> np.ndarray:
        """Frames pushed since reset, per slot: a copy of the host mirror (no device read)."""
        return self._counts.copy()

    def _lift(self, ids_d, K: int, back: int, n_out: int) -> torch.Tensor:
        """Current windows of the K slots -> one forward -> rows ``clamp(L - 1 - back + r, 0, L - 1)``, r < n_out, of each: [K, n_out, 17, 3]."""
        lib, T, S, halves = self._lib, self.T, self.slots, (2 if self.flip else 1)
        slots_p = ids_d.data_ptr() if ids_d is not None else None
        x = torch.empty((halves * K, T, 17, 3), dtype=torch.float32, device=self.device)
        _lib.check(lib.kasf_stream_windows(self._ring.data_ptr(), self._count.data_ptr(), slots_p, K, S, T, self._width.data_ptr(),
                                           self._height.data_ptr(), self._r_tab.data_ptr(), int(self.flip), x.data_ptr(), _args.stream()))
        pred = _forward_windows(self.model, x, K, halves, K)
        out = torch.empty((K, n_out, 17, 3), dtype=torch.float32, device=self.device)
        _lib.check(lib.kasf_stream_emit(pred.data_ptr(), int(self.flip), self._count.data_ptr(), slots_p, K, S, T, self._fp_tab.data_ptr(), back, n_out,
                                        out.data_ptr(), _args.stream()))
        return out

    def push(self, keypoints, slots=None) -> torch.Tensor:
        """One new frame per slot: ``keypoints`` [slots,17,3] (every slot, in order) or, with ``slots=`` (distinct host integers), [K,17,3] for those
        slots; float32 pixel x, y, confidence, numpy or torch, CPU or on the model's GPU.  Returns CUDA fp32 [K,17,3]: per pushed slot, frame
        ``max(L - 1 - lag, 0)`` of its current window's lift (while the slot has at most ``lag`` frames that is its first frame, not final yet)."""
        kp = float_rows(keypoints, self.device, "StreamLifter.push")
        ids = slot_ids(slots, self.slots, "StreamLifter.push")
        K = self.slots if ids is None else int(ids.size)
        if kp.dim() != 3 or tuple(kp.shape) != (K, 17, 3):
            raise ValueError(f"StreamLifter.push: expected keypoints [{K},17,3] (one frame per pushed slot), got {tuple(kp.shape)}")
        if K == 0:
            return torch.empty((0, 17, 3), dtype=torch.float32, device=self.device)
        frames = kp.to(self.device).contiguous()               # a copy when it comes from the host; on the device the kernel only reads it
        ids_d = torch.from_numpy(ids).to(self.device) if ids is not None else None
        with torch.no_grad():
            if self._coco:
                frames = convert_frames(frames)
            _lib.check(self._lib.kasf_stream_push(frames.data_ptr(), ids_d.data_ptr() if ids_d is not None else None, K, self.slots, self.T,
                                                  self._ring.data_ptr(), self._count.data_ptr(), _args.stream()))
            if ids is None:
                self._counts += 1
            else:
                self._counts[ids] += 1
            return self._lift(ids_d, K, self.lag, 1).view(K, 17, 3)

    def push_heatmaps(self, heatmaps, center=None, scale=None, *, boxes=None, aspect=None, refine: bool = True, slots=None, flipped=None,
                      shift: bool = True, pairs=None, decode: str = "quarter", kernel=None, sigma=None, udp=None) -> torch.Tensor:
        """One new frame per slot straight from the pose network: ``heatmaps`` [K,17,H,W] (float32, float16 or bfloat16; normally the network's output
        on the model's GPU, read in place) with ``center`` / ``scale`` [K,2] or ``boxes`` [K,4] and ``aspect`` as ``heatmaps_to_keypoints`` takes them,
        decoded on the device and pushed: what ``push`` returns for ``heatmaps_to_keypoints(..., layout="h36m")`` of them (for the COCO result on a
        ``layout="coco"`` lifter, which is the same frames).  Two launches in front of ``push``'s, no host round trip.  Nothing is filtered: a map that
        holds a NaN gives a NaN score (and possibly coordinates) in the ring, as pushing those keypoints would.  ``flipped`` / ``shift`` / ``pairs``: the
        flip test, and ``decode`` / ``kernel`` / ``sigma`` / ``udp``: the DARK / UDP sub-pixel decode, as ``heatmaps_to_keypoints`` takes them (still one decode
        launch)."""
        who = "StreamLifter.push_heatmaps"
        hm, parts, kind, aspect = check_heatmap_args(heatmaps, center, scale, boxes, aspect, who)
        flip = check_flip_args(hm, flipped, shift, pairs, who)
        dark = check_decode_args(hm, decode, kernel, sigma, udp, refine, who)
        ids = slot_ids(slots, self.slots, who)
        K = self.slots if ids is None else int(ids.size)
        if hm.dim() != 4 or hm.shape[0] != K:
            raise ValueError(f"{who}: expected heatmaps [{K},17,H,W] (one person per pushed slot), got {tuple(hm.shape)}")
        return self.push(_decode_on(self.device, hm, parts, kind, aspect, refine, not self._coco, who, flip, dark), slots=slots)

    def tail(self, slots=None) -> torch.Tensor:
        """The ``lag`` frames ``push`` has not emitted yet, from the current windows, for the end of a track: [K,lag,17,3], row r = frame
        ``clamp(L - lag + r, 0, L - 1)`` of the window's lift.  One forward, state unchanged; ``lag == 0`` gives an empty [K,0,17,3] without a forward."""
        ids = slot_ids(slots, self.slots, "StreamLifter.tail")
        K = self.slots if ids is None else int(ids.size)
        if np.any((self._counts if ids is None else self._counts[ids]) < 1):
            raise ValueError("StreamLifter.tail: a slot without frames has no window (push first)")
        if K == 0 or self.lag == 0:
            return torch.empty((K, self.lag, 17, 3), dtype=torch.float32, device=self.device)
        ids_d = torch.from_numpy(ids).to(self.device) if ids is not None else None
        with torch.no_grad():
            return self._lift(ids_d, K, self.lag - 1, self.lag)

    def reset(self, slots=None) -> None:
        """The slots start a new history (``reset()``: all of them).  Only the counts are zeroed: every ring position a window reads is written first."""
        ids = slot_ids(slots, self.slots, "StreamLifter.reset")
        if ids is None:
            self._count.zero_()
            self._counts[:] = 0
        elif ids.size:
            self._count.index_fill_(0, torch.from_numpy(ids.astype(np.int64)).to(self.device), 0)
            self._counts[ids] = 0

    def replay(self, track, width=None, height=None) -> torch.Tensor:
        """A recorded track, [N,17,3] or [P,N,17,3], tick by tick and then ``tail``, through a temporary state of P slots with this lifter's model, flip and
        lag (its live slots are not touched): CUDA fp32 of the track's shape, frame f taken from the window after push number ``min(f + lag + 1, N)``.
        For N <= T and lag = T - 1 that is ``lift_track(model, track, ...)``.  The resolution is the lifter's when it was built with one value; otherwise
        ``width=`` and ``height=`` (one value or one per track) are required."""
        kp = float_rows(track, self.device, "StreamLifter.replay")
        if kp.dim() not in (3, 4) or tuple(kp.shape[-2:]) != (17, 3):
            raise ValueError(f"StreamLifter.replay: expected a track [N,17,3] or [P,N,17,3], got {tuple(kp.shape)}")
        if (width is None) != (height is None):
            raise ValueError("StreamLifter.replay: width and height go together")
        if width is None:
            if self._one_resolution is None:
                raise ValueError("StreamLifter.replay: this lifter has one resolution per slot; pass width= and height= for the track(s)")
            width, height = self._one_resolution
        lead = tuple(kp.shape[:-2])
        kp4 = kp if kp.dim() == 4 else kp.unsqueeze(0)
        P, N, lag = int(kp4.shape[0]), int(kp4.shape[1]), self.lag
        out = torch.empty((P, N, 17, 3), dtype=torch.float32, device=self.device)
        if P == 0 or N == 0:
            if P > 0:
                _per_row(width, P, "width", "StreamLifter", "slot"), _per_row(height, P, "height", "StreamLifter", "slot")
            return out.view(lead + (17, 3))
        temp = StreamLifter(self.model, width, height, slots=P, flip=self.flip, lag=lag, layout=self.layout, _tables=self._tables)
        ticks = kp4.to(self.device).transpose(0, 1).contiguous()   # [N,P,17,3]: one upload, every tick reads its frame in place
        for f in range(N):
            pose = temp.push(ticks[f])
            if f >= lag:
                out[:, f - lag] = pose
        if lag > 0:
            m = min(lag, N)
            out[:, N - m:] = temp.tail()[:, lag - m:]
        return out.view(lead + (17, 3))
