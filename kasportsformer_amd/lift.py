"""Lifting a 2-D keypoint track to 3-D poses on the GPU: the demo's stage 2 (demo/demo.py:194-254, ``lift_3d_pose``) without the detectors.

    poses = lift_track(model, keypoints, width, height)          # keypoints [N,17,3] or [P,N,17,3] pixels + confidence -> [..., 17, 3]
    poses = lift_tracks(model, [kp_0, kp_1, ...], width, height) # tracks [N_i,17,3] of different lengths -> a list of [N_i,17,3], one batch

The demo cuts the track into T-frame clips (``turn_into_clips`` / ``resample``, demo.py:132-156), normalises them
(``normalize_screen_coordinates``, demo/lib/utils.py:16-20), runs two forwards per clip (plain and ``flip_data``-mirrored), averages the
flip-TTA pair, zeroes the root and keeps the original frames of the resampled tail clip.  Here one kernel cuts, normalises and mirrors
every window of every person (``kasf_lift_windows``), the forward runs on stacked batches of windows, and one kernel merges the pair and
puts the frames back on the track (``kasf_lift_stitch``).  Two demo bugs are not reproduced: ``flip_data`` flips its argument in place
(demo.py:227: both forwards see the mirrored clip), and ``turn_into_clips`` raises ``UnboundLocalError`` when N > T and N % T == 0.

``stride < T`` selects overlapping windows (not in the demo): each frame is the mean over the windows that cover it.

``lift_tracks`` takes tracks of different lengths (one per tracked player): each is cut by its own plan, the windows of all of them go through
the forward together (``kasf_lift_windows_ragged`` / ``kasf_lift_stitch_ragged``), and each track gets what ``lift_track`` gives it alone.

    python -m kasportsformer_amd.lift --config X.yaml --checkpoint best.pth --keypoints keypoints2d.pkl --width 1280 --height 720 --out poses3d.npy

``--online [--lag D]`` replays the file tick by tick through ``kasportsformer_amd.stream.StreamLifter`` (the lift of live streams) instead.

``layout="coco"`` (``--layout coco``) takes the keypoints as a COCO-17 detector writes them and converts them on the device first
(``kasportsformer_amd.pose.coco_to_h36m``); ``--smooth [--smooth-rate] [--smooth-min-cutoff] [--smooth-beta] [--smooth-min-score]`` sends the keypoints
through the One-Euro filter first (``kasportsformer_amd.smooth.smooth_tracks``), offline and ``--online`` alike; ``--refine [--refine-min-score] [--refine-max-gap] [--refine-sigma]`` takes that place for a recorded
track (``kasportsformer_amd.refine.refine_tracks``: occlusion gaps filled from both sides, then a zero-phase Gaussian; not with ``--smooth``, not with ``--online``)
and ``--refine-poses`` runs the same over the lifted poses, before ``--fix-bones``; ``--fix-bones [--fix-bones-symmetric]`` gives every bone of a track one length
(``kasportsformer_amd.bones.fix_bone_lengths`` over the final poses, before ``--world``); ``--place --camera FX,FY,CX,CY [--place-lengths table.npy]
[--place-iterations] [--place-delta]`` then puts every pose where its player stood in front of the camera (``kasportsformer_amd.place.place_poses``, after
``--fix-bones`` and ``--refine-poses``, before ``--world``; not with ``--world-unit``; an ``.npz`` output also gets ``root_i`` and ``place_state_i`` per track;
``--camera-distortion K1,K2,P1,P2,K3`` sends the keypoints it is given through ``kasportsformer_amd.triangulate.undistort_keypoints`` first); ``--world [--world-floor] [--world-unit]`` sends the poses through ``poses_to_world`` before they are written.
"""
from __future__ import annotations

import argparse
import io
import pickle

import numpy as np
import torch

from . import _args, _lib
from ._tracks import float_rows, pack, recorded_parts, split, track_offsets
from .pose import check_layout, convert_frames, poses_to_world


def demo_resample(n_frames: int, target_frame: int) -> np.ndarray:
    """demo.py:132-136: ``target_frame`` indices into ``n_frames`` frames (float64 linspace without the end point, floor, clip)."""
    even = np.linspace(0, n_frames, num=target_frame, endpoint=False)
    return np.clip(np.floor(even), a_min=0, a_max=n_frames - 1).astype(np.int32)


def window_plan(n: int, T: int, stride: int | None = None):
    """Windows of ``T`` frames over an ``n``-frame track: ``(starts [W] int64, lengths [W] int64, resample [T] int32 or None, first_pos [L] int32 or None)``.

    ``stride == T`` (default): the demo's clips -- starts 0, T, 2T, ...; a last window of L < T frames is resampled to T through
    ``resample = demo_resample(L, T)``, and ``first_pos[j]`` is the first t with ``resample[t] == j`` (the demo's ``downsample``,
    ``np.unique(r, return_index=True)[1]``).  ``stride < T`` and n > T: starts 0, s, 2s, ... while ``start + T < n``, plus ``n - T``; all full."""
    stride = T if stride is None else int(stride)
    if T < 1 or not 1 <= stride <= T:
        raise ValueError(f"window_plan: need T >= 1 and 1 <= stride <= T, got T={T} stride={stride}")
    if n < 0:
        raise ValueError("window_plan: n must be >= 0")
    if n == 0:
        starts = np.zeros(0, np.int64)
    elif n <= T:
        starts = np.zeros(1, np.int64)
    elif stride == T:
        starts = np.arange(0, n, T, dtype=np.int64)
    else:
        starts = np.concatenate((np.arange(0, n - T, stride, dtype=np.int64), [n - T])).astype(np.int64)
    lengths = np.minimum(n - starts, T).astype(np.int64)
    resample = first_pos = None
    if len(lengths) and lengths[-1] < T:
        L = int(lengths[-1])
        resample = demo_resample(L, T)
        first_pos = np.unique(resample, return_index=True)[1].astype(np.int32)
    return starts, lengths, resample, first_pos


def ragged_plan(lengths, T: int, stride: int | None = None):
    """The window plans of many tracks, ``window_plan`` track by track: ``(win_first [P+1] int64, resample [P,T] int32, first_pos [P,T] int32)``.
    Track p owns windows ``win_first[p] .. win_first[p+1] - 1`` of the call; rows p of ``resample`` / ``first_pos`` hold its tables (``first_pos``
    in the first L entries) when its plan has a resampled window, and zeros, which the kernels never read, otherwise."""
    window_plan(0, T, stride)                               # refuses a bad T or stride even without tracks
    lengths = [int(n) for n in lengths]
    win_first = np.zeros(len(lengths) + 1, np.int64)
    resample = np.zeros((len(lengths), T), np.int32)
    first_pos = np.zeros((len(lengths), T), np.int32)
    plans = {}
    for p, n in enumerate(lengths):
        if n not in plans:
            plans[n] = window_plan(n, T, stride)
        starts, _, r, fp = plans[n]
        win_first[p + 1] = win_first[p] + len(starts)
        if r is not None:
            resample[p], first_pos[p, :len(fp)] = r, fp
    return win_first, resample, first_pos


def _model_device(model, who: str = "lift_track") -> torch.device:
    dev = model._flat.device
    if dev.type != "cuda":
        raise RuntimeError(f"{who}: the model must be on the GPU (model.cuda()); kasportsformer_amd has no CPU path")
    return dev


def _track(keypoints, device) -> torch.Tensor:
    kp = float_rows(keypoints, device, "lift_track")
    if kp.dim() not in (3, 4) or tuple(kp.shape[-2:]) != (17, 3):
        raise ValueError(f"lift_track: expected keypoints [N,17,3] or [P,N,17,3], got {tuple(kp.shape)}")
    return kp.to(device).contiguous()            # a copy when it comes from the host; on the device the kernels only read it


def lift_track(model, keypoints, width, height, *, stride=None, flip: bool = True, max_windows: int = 1024, layout: str = "h36m") -> torch.Tensor:
    """3-D poses of a 2-D keypoint track: ``keypoints`` [N,17,3] or [P,N,17,3] float32 (pixel x, y, confidence; numpy or torch, CPU or
    GPU, never modified) -> CUDA fp32 [N,17,3] / [P,N,17,3] in the model's output space with the root joint at zero (the demo's
    ``output_3D`` before ``camera_to_world``).  T is ``model.n_frames``; ``stride`` defaults to T (the demo's clips).  The forward runs in
    eval mode without autograd, the plain and mirrored views of each window in one stacked batch, at most ``max_windows`` windows
    (2 * ``max_windows`` clips with ``flip``) per call; ``model.training`` is restored afterwards.  ``layout="coco"``: the keypoints are COCO-17
    (pixel x, y, score) and go through ``coco_to_h36m`` on the device first; any other value but "h36m" raises ``ValueError``."""
    coco = check_layout(layout, "lift_track")
    device = _model_device(model)
    kp = _track(keypoints, device)
    lead = tuple(kp.shape[:-2])
    kp4 = kp if kp.dim() == 4 else kp.unsqueeze(0)
    P, n = int(kp4.shape[0]), int(kp4.shape[1])
    T = int(model.n_frames)
    stride = _stride(T, stride, max_windows, "lift_track")
    if not (float(width) > 0 and float(height) > 0):
        raise ValueError("lift_track: width and height must be positive")
    if P == 0 or n == 0:
        return torch.empty(lead + (17, 3), dtype=torch.float32, device=device)
    lib = _lib.load()
    starts, _, resample, first_pos = window_plan(n, T, stride)
    W = len(starts)
    if lib.kasf_lift_window_count(n, T, stride) != W:
        raise _lib.KasfError("lift_track: the library's window count disagrees with window_plan (stale build?)")
    r_dev = torch.from_numpy(resample).to(device) if resample is not None else None
    fp_dev = torch.from_numpy(first_pos).to(device) if first_pos is not None else None
    halves, PW = (2 if flip else 1), P * W
    with torch.no_grad():
        if coco:
            kp4 = convert_frames(kp4)
        x = torch.empty((halves * PW, T, 17, 3), dtype=torch.float32, device=device)
        _lib.check(lib.kasf_lift_windows(kp4.data_ptr(), P, n, float(width), float(height), T, stride,
                                         r_dev.data_ptr() if r_dev is not None else None, int(flip), x.data_ptr(), _args.stream()))
        pred = _forward_windows(model, x, PW, halves, int(max_windows))
        poses = torch.empty((P, n, 17, 3), dtype=torch.float32, device=device)
        _lib.check(lib.kasf_lift_stitch(pred.data_ptr(), int(flip), P, n, T, stride, fp_dev.data_ptr() if fp_dev is not None else None,
                                        poses.data_ptr(), _args.stream()))
    return poses.view(lead + (17, 3))


def _stride(T: int, stride, max_windows, who: str) -> int:
    """The ``stride`` (None: T) and ``max_windows`` of a call, checked -> the stride."""
    stride = T if stride is None else int(stride)
    if not 1 <= stride <= T:
        raise ValueError(f"{who}: stride must be in [1, T={T}], got {stride}")
    if int(max_windows) < 1:
        raise ValueError(f"{who}: max_windows must be >= 1")
    return stride


def _per_row(value, count: int, name: str, who: str, unit: str) -> np.ndarray:
    """``width`` / ``height``: one value for every track (slot, stream: ``unit``) or one per track -> float32 [count] (what the C entry points receive)."""
    v = np.asarray(value.detach().cpu() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
    if v.ndim == 0:
        v = np.full(count, v)
    elif v.shape != (count,):
        raise ValueError(f"{who}: {name} must be one value or one per {unit} ({count}), got shape {v.shape}")
    v = v.astype(np.float32)
    if not np.all(v > 0):
        raise ValueError(f"{who}: width and height must be positive")
    return v


_TORCH_DTYPE = {np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


def _upload(device, *arrays):
    """Small host arrays in one host-to-device copy: a device tensor per array (views of one buffer at 8-byte aligned offsets)."""
    at = np.cumsum([0] + [(a.nbytes + 7) // 8 * 8 for a in arrays])
    buf = np.zeros(int(at[-1]), np.uint8)
    for a, o in zip(arrays, at):
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    dev = torch.from_numpy(buf).to(device)
    return [dev[o:o + a.nbytes].view(_TORCH_DTYPE[a.dtype]).view(a.shape) for a, o in zip(arrays, at)]


def _forward_windows(model, x, windows: int, halves: int, max_windows: int) -> torch.Tensor:
    """The eval-mode forward of stacked windows x [halves * windows, T, 17, 3] (plain half, then mirrored): one batch, or chunks of at most
    ``max_windows`` windows in window order with both halves of a chunk in one forward; ``model.training`` is restored."""
    was_training = model.training
    model.eval()
    try:
        if windows <= max_windows:
            return model(x)
        pred = torch.empty_like(x)
        for a in range(0, windows, max_windows):
            b = min(a + max_windows, windows)
            idx = [slice(h * windows + a, h * windows + b) for h in range(halves)]
            out = model(torch.cat([x[i] for i in idx]) if halves == 2 else x[idx[0]])
            for h, i in enumerate(idx):
                pred[i].copy_(out[h * (b - a):(h + 1) * (b - a)])
        return pred
    finally:
        model.train(was_training)


def lift_tracks(model, tracks, width, height, *, stride=None, flip: bool = True, max_windows: int = 1024, offsets=None, layout: str = "h36m"):
    """3-D poses of many 2-D keypoint tracks of different lengths in one batched lift: ``tracks`` a sequence of [N_i,17,3] float32 arrays
    (numpy or torch, CPU or on the model's GPU, any N_i >= 0, never modified) -> a list of CUDA fp32 [N_i,17,3] tensors, views of one packed
    result.  With ``offsets`` (integers [P+1]: 0, non-decreasing, ending at the packed length), ``tracks`` is one packed [sum N_i,17,3] array,
    track i its rows offsets[i] .. offsets[i+1] - 1, and the result is one packed tensor too.  ``width`` / ``height``: one value, or one per
    track (cameras of different resolutions).

    Each track is cut by its own plan (``window_plan``; ``stride`` as in ``lift_track``), and the windows of all tracks run through the forward
    together: one stacked batch, or chunks of at most ``max_windows`` windows in track order (a chunk may split a track).  Track i's poses are
    ``lift_track(model, tracks[i], ...)``'s -- bit for bit in fp32, where an eval forward computes every clip alone.  Eval mode without
    autograd; ``model.training`` is restored afterwards.  ``layout="coco"``: the tracks are COCO-17 keypoints, converted on the device (one launch over
    the packed frames) before they are cut.  Bad shapes, dtypes, devices, strides, layouts and resolution counts raise before any kernel runs."""
    coco = check_layout(layout, "lift_tracks")
    device = _model_device(model, "lift_tracks")
    T = int(model.n_frames)
    stride = _stride(T, stride, max_windows, "lift_tracks")
    parts, as_list = recorded_parts(tracks, offsets, "lift_tracks", lambda a: float_rows(a, device, "lift_tracks"), "17,3", False, exact=True)
    off = track_offsets(parts, offsets, as_list, "lift_tracks")
    P = len(off) - 1
    w32, h32 = _per_row(width, P, "width", "lift_tracks", "track"), _per_row(height, P, "height", "lift_tracks", "track")
    lengths = np.diff(off)
    win_first, resample, first_pos = ragged_plan(lengths, T, stride)
    frames, windows = int(off[-1]), int(win_first[-1])
    lib = _lib.load()
    c_first = np.empty(P + 1, np.int64)
    if (lib.kasf_lift_ragged_plan(lengths.ctypes.data, P, T, stride, c_first.ctypes.data) != windows
            or not np.array_equal(c_first, win_first)):
        raise _lib.KasfError("lift_tracks: the library's window plan disagrees with ragged_plan (stale build?)")
    if as_list and P == 0:
        return []
    packed = pack(parts, as_list, device)
    poses = torch.empty((frames, 17, 3), dtype=torch.float32, device=device)
    if windows > 0:
        off_d, wf_d, w_d, h_d, r_d, fp_d = _upload(device, off, win_first, w32, h32, resample, first_pos)
        halves = 2 if flip else 1
        with torch.no_grad():
            if coco:
                packed = convert_frames(packed)
            x = torch.empty((halves * windows, T, 17, 3), dtype=torch.float32, device=device)
            _lib.check(lib.kasf_lift_windows_ragged(packed.data_ptr(), off_d.data_ptr(), wf_d.data_ptr(), P, frames, windows, w_d.data_ptr(),
                                                    h_d.data_ptr(), T, stride, r_d.data_ptr(), int(flip), x.data_ptr(), _args.stream()))
            pred = _forward_windows(model, x, windows, halves, int(max_windows))
            _lib.check(lib.kasf_lift_stitch_ragged(pred.data_ptr(), int(flip), off_d.data_ptr(), wf_d.data_ptr(), P, frames, windows, T, stride,
                                                   fp_d.data_ptr(), poses.data_ptr(), _args.stream()))
    return split(poses, off) if as_list else poses


class _KeypointUnpickler(pickle.Unpickler):
    """``keypoints2d.pkl`` (the demo's ``detect_2d_pose`` output) holds one numpy array: only the globals an ndarray pickle names may be loaded
    (numpy 1.x and 2.x module paths, protocols 2-5).  Any other global -- a numpy function included -- is refused before it can be called."""

    ALLOWED = {("numpy", "ndarray"), ("numpy", "dtype"),
               ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"),
               ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
               ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer"),
               ("_codecs", "encode")}                              # protocol 2 writes the raw bytes as _codecs.encode(str, 'latin1')

    def find_class(self, module, name):
        if (module, name) in self.ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"keypoint file references {module}.{name}: only the globals of a numpy array pickle are allowed")


def _numeric(kp, what) -> np.ndarray:
    if not isinstance(kp, np.ndarray) or kp.dtype.hasobject:
        raise TypeError(f"{what}: expected a numeric numpy array, got {type(kp).__name__} {getattr(kp, 'dtype', '')}")
    return np.ascontiguousarray(kp, dtype=np.float32)


def load_keypoints(path: str):
    """[P,N,17,3] (or [N,17,3]) float32 keypoints from a ``.npy`` file (no pickles) or a ``.pkl`` file of numpy arrays only.  Tracks of
    different lengths -- a ``.npz`` (its arrays in file order; no pickles) or a ``.pkl`` holding a list or tuple of arrays (lists and tuples
    are pickle opcodes, not globals: the unpickler admits nothing new) -- come back as a list of float32 arrays."""
    if str(path).endswith(".npy"):
        kp = np.load(path, allow_pickle=False)
    elif str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return [_numeric(z[k], f"{path}:{k}") for k in z.files]
    else:
        with open(path, "rb") as f:
            kp = _KeypointUnpickler(io.BytesIO(f.read())).load()
        if isinstance(kp, (list, tuple)):
            return [_numeric(a, path) for a in kp]
    return _numeric(kp, path)


def _parse(argv=None):
    """The command line of ``python -m kasportsformer_amd.lift`` (no device needed)."""
    ap = argparse.ArgumentParser(prog="python -m kasportsformer_amd.lift", description="Lift a 2-D keypoint track to 3-D poses (demo.py stage 2).")
    ap.add_argument("--config", required=True, help="model yaml (configs/*.yaml)")
    ap.add_argument("--checkpoint", required=True, help="checkpoint written by checkpoint_save or the reference's training script")
    ap.add_argument("--keypoints", required=True, help="keypoints2d.pkl ([P,N,17,3], the demo's detect_2d_pose output) or .npy; tracks of different "
                                                       "lengths: an .npz of [N_i,17,3] arrays (file order) or a .pkl of a list of them")
    ap.add_argument("--width", type=float, required=True, help="frame width in pixels")
    ap.add_argument("--height", type=float, required=True, help="frame height in pixels")
    ap.add_argument("--stride", type=int, default=None, help="window stride (default: T, the demo's clips; < T: overlapping windows averaged)")
    ap.add_argument("--no-flip", action="store_true", help="skip the flip-TTA pair")
    ap.add_argument("--compute-dtype", choices=("bf16", "fp32"), default=None, help="default: the yaml's compute_dtype, else bf16")
    ap.add_argument("--max-windows", type=int, default=1024)
    ap.add_argument("--online", action="store_true", help="replay the track(s) tick by tick through StreamLifter (kasportsformer_amd.stream): frame f "
                                                          "from the sliding window of the T frames up to f + LAG; not with --stride")
    ap.add_argument("--lag", type=int, default=0, help="--online: frames of look-ahead, in [0, T - 1] (default 0: every pose from the frames up to its own)")
    ap.add_argument("--layout", choices=("h36m", "coco"), default="h36m", help="joint layout of the keypoints: h36m (default; the demo's keypoints2d.pkl) or "
                                                                               "coco (COCO-17 x, y, score as a detector writes them: converted on the device)")
    ap.add_argument("--world", action="store_true", help="write world-space poses: the demo's camera_to_world rotation (demo.py:243-245)")
    ap.add_argument("--world-floor", action="store_true", help="--world: put each frame's lowest joint at z = 0 (demo.py:246)")
    ap.add_argument("--world-unit", action="store_true", help="--world: divide each frame by its largest value (demo.py:247-248), after --world-floor")
    ap.add_argument("--smooth", action="store_true", help="run the One-Euro filter (kasportsformer_amd.smooth_tracks) over the keypoints before the lift: steadier "
                                                          "coordinates, joints scored below --smooth-min-score hold their last estimate")
    ap.add_argument("--smooth-rate", type=float, default=None, help="--smooth: frames per second of the track (default 30)")
    ap.add_argument("--smooth-min-cutoff", type=float, default=None, help="--smooth: cutoff at rest in Hz (default 1.0; lower: steadier, more lag)")
    ap.add_argument("--smooth-beta", type=float, default=None, help="--smooth: cutoff gained per pixel / s of speed (default 0.01; higher: less lag in motion)")
    ap.add_argument("--smooth-min-score", type=float, default=None, help="--smooth: a joint scored below this holds (default 0.3)")
    ap.add_argument("--refine", action="store_true", help="fill the gaps of joints scored below --refine-min-score from the frames on both sides and smooth with a "
                                                          "zero-phase Gaussian (kasportsformer_amd.refine_tracks) over the keypoints before the lift; a recorded "
                                                          "track only: not with --smooth, not with --online")
    ap.add_argument("--refine-min-score", type=float, default=None, help="--refine: a joint scored below this is filled (default 0.3)")
    ap.add_argument("--refine-max-gap", type=int, default=None, help="--refine: the longest run of frames that is filled, in [0, 64] (default 15)")
    ap.add_argument("--refine-sigma", type=float, default=None, help="--refine: the Gaussian's sigma in frames (default 2.0; a starting point, not tuned on footage)")
    ap.add_argument("--refine-poses", action="store_true", help="run refine_tracks over the lifted poses as well (no score: only a NaN gates a joint), before "
                                                                "--fix-bones; not with --online")
    ap.add_argument("--fix-bones", action="store_true", help="give every bone of a track one length, the track's lower median (kasportsformer_amd.fix_bone_lengths), "
                                                             "over the final poses and before --world")
    ap.add_argument("--fix-bones-symmetric", action="store_true", help="--fix-bones: left / right partner bones get their mean")
    ap.add_argument("--place", action="store_true", help="place every pose in camera space from its keypoints and --camera (kasportsformer_amd.place_poses), "
                                                         "after --refine-poses and --fix-bones, before --world; an .npz output also gets root_i and place_state_i")
    ap.add_argument("--camera", default=None, help="--place: the pinhole intrinsics FX,FY,CX,CY in pixels (a lens with distortion: --camera-distortion)")
    ap.add_argument("--camera-distortion", default=None, help="--place: the lens' Brown-Conrady coefficients K1,K2,P1,P2,K3 (OpenCV's order): the keypoints "
                                                              "given to the placement are undistorted first (kasportsformer_amd.undistort_keypoints)")
    ap.add_argument("--place-lengths", default=None, help="--place: an .npy of the sixteen bone lengths in metres (0 skips a bone): the roots come out in metres")
    ap.add_argument("--place-iterations", type=int, default=None, help="--place: rounds of Cauchy re-weighting, in [0, 8] (default 4)")
    ap.add_argument("--place-delta", type=float, default=None, help="--place: the re-weighting's scale in pixels (default 3.0; a starting point, not tuned on footage)")
    ap.add_argument("--out", required=True, help="output .npy of [P,N,17,3] (or [N,17,3]) float32 poses; tracks of different lengths: an .npz "
                                                 "of track_0 ... track_{P-1}")
    args = ap.parse_args(argv)
    smooth_defaults = dict(smooth_rate=30.0, smooth_min_cutoff=1.0, smooth_beta=0.01, smooth_min_score=0.3)
    if not args.smooth and any(getattr(args, k) is not None for k in smooth_defaults):
        ap.error("--smooth-rate, --smooth-min-cutoff, --smooth-beta and --smooth-min-score belong to --smooth")
    for k, v in smooth_defaults.items():
        if getattr(args, k) is None:
            setattr(args, k, v)
    refine_defaults = dict(refine_min_score=0.3, refine_max_gap=15, refine_sigma=2.0)
    if not args.refine and any(getattr(args, k) is not None for k in refine_defaults):
        ap.error("--refine-min-score, --refine-max-gap and --refine-sigma belong to --refine")
    for k, v in refine_defaults.items():
        if getattr(args, k) is None:
            setattr(args, k, v)
    if args.refine and args.smooth:
        ap.error("--refine and --smooth both clean up the keypoints before the lift: give one of them")
    if (args.refine or args.refine_poses) and args.online:
        ap.error("--refine and --refine-poses are zero-phase: they need the frames after, which --online does not have (--smooth is the live filter)")
    if args.fix_bones_symmetric and not args.fix_bones:
        ap.error("--fix-bones-symmetric belongs to --fix-bones")
    if args.online and args.stride is not None:
        ap.error("--online lifts the sliding window of every tick: it takes no --stride")
    if args.lag and not args.online:
        ap.error("--lag belongs to --online")
    if (args.world_floor or args.world_unit) and not args.world:
        ap.error("--world-floor and --world-unit belong to --world")
    place_defaults = dict(place_iterations=4, place_delta=3.0)
    if not args.place and (args.camera is not None or args.place_lengths is not None or any(getattr(args, k) is not None for k in place_defaults)):
        ap.error("--camera, --place-lengths, --place-iterations and --place-delta belong to --place")
    if not args.place and args.camera_distortion is not None:
        ap.error("--camera-distortion belongs to --place")
    for k, v in place_defaults.items():
        if getattr(args, k) is None:
            setattr(args, k, v)
    if args.place:
        if args.camera is None:
            ap.error("--place needs --camera FX,FY,CX,CY")
        if args.world_unit:
            ap.error("--place is refused with --world-unit, which divides every frame by its largest value: the placement would be divided away")
        try:
            camera = [float(v) for v in args.camera.split(",")]
        except ValueError:
            camera = []
        if len(camera) != 4 or not all(np.isfinite(np.float32(v)) for v in camera) or not (camera[0] > 0 and camera[1] > 0):
            ap.error(f"--camera must be four finite numbers FX,FY,CX,CY with FX, FY > 0, got {args.camera!r}")
        args.camera = np.array(camera, np.float32)
        if args.camera_distortion is not None:
            try:
                lens = [float(v) for v in args.camera_distortion.split(",")]
            except ValueError:
                lens = []
            if len(lens) != 5 or not all(abs(v) <= float(np.finfo(np.float32).max) for v in lens):         # false for a NaN: finite as the device's fp32
                ap.error(f"--camera-distortion must be five finite numbers K1,K2,P1,P2,K3, got {args.camera_distortion!r}")
            args.camera_distortion = np.array(lens, np.float32)
        if not 0 <= args.place_iterations <= 8:
            ap.error("--place-iterations must be in [0, 8]")
        if not (np.isfinite(args.place_delta) and args.place_delta > 0):
            ap.error("--place-delta must be finite and > 0 pixels")
    return args


def main(argv=None):
    args = _parse(argv)
    place_table = None
    if args.place_lengths is not None:                 # refused before the model is loaded
        from .place import load_bone_table
        place_table = load_bone_table(args.place_lengths)

    import yaml
    from .checkpoint import checkpoint_load
    from .model import load_model
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    if args.compute_dtype is not None:
        cfg["compute_dtype"] = args.compute_dtype
    model = load_model(cfg).cuda()
    checkpoint_load(args.checkpoint, model)
    keypoints = load_keypoints(args.keypoints)
    if args.smooth:                                # every track from an empty state, on the model's GPU; the lifts below take the result where it is
        from .smooth import smooth_tracks
        keypoints = smooth_tracks(keypoints, score=True, rate=args.smooth_rate, min_cutoff=args.smooth_min_cutoff, beta=args.smooth_beta,
                                  min_score=args.smooth_min_score, device=_model_device(model))
    if args.refine:                                # in the place --smooth has: one launch over every track, on the model's GPU
        from .refine import refine_tracks
        keypoints = refine_tracks(keypoints, score=True, min_score=args.refine_min_score, max_gap=args.refine_max_gap, sigma=args.refine_sigma,
                                  device=_model_device(model))

    extras = {}                                        # --place: root_i and place_state_i of an .npz output

    def final(poses, kp, i=None):
        """The stages behind the lift over one track's poses; kp: the keypoints they were lifted from, as the lift took them."""
        if args.refine_poses:                          # poses carry no score: only a joint that is not finite is filled
            from .refine import refine_tracks
            poses = refine_tracks(poses, score=False)
        if args.fix_bones:                             # one track [N,17,3], or [P,N,17,3]: every track its own medians
            from .bones import fix_bone_lengths
            poses = fix_bone_lengths(poses, symmetric=args.fix_bones_symmetric)
        if args.place:                                 # the keypoints in the layout the model saw; frames that cannot be placed come out NaN
            from .place import place_poses
            from .pose import coco_to_h36m
            kp = coco_to_h36m(kp, device=poses.device) if args.layout == "coco" else kp
            if args.camera_distortion is not None:     # the placement's camera is a pinhole: it gets the keypoints that one would have seen
                from .triangulate import undistort_keypoints
                kp = undistort_keypoints(kp, args.camera, args.camera_distortion, device=poses.device)
            placed = place_poses(poses, kp, args.camera, metric_lengths=place_table,
                                 iterations=args.place_iterations, delta=args.place_delta, device=poses.device)
            poses = placed.poses
            if i is not None:
                extras[f"root_{i}"], extras[f"place_state_{i}"] = placed.root.cpu().numpy(), placed.state.cpu().numpy()
        return poses_to_world(poses, floor=args.world_floor, unit=args.world_unit) if args.world else poses

    if args.online:
        from .stream import StreamLifter
        lifter = StreamLifter(model, args.width, args.height, slots=1, flip=not args.no_flip, lag=args.lag, layout=args.layout)
        if isinstance(keypoints, list):
            np.savez(args.out, **{f"track_{i}": final(lifter.replay(k), k, i).cpu().numpy() for i, k in enumerate(keypoints)}, **extras)
            print(f"replayed {len(keypoints)} tracks ({sum(len(k) for k in keypoints)} frames) tick by tick, lag {args.lag} -> {args.out}")
            return
        poses = final(lifter.replay(keypoints), keypoints)
        np.save(args.out, poses.cpu().numpy())
        print(f"replayed {keypoints.shape} tick by tick, lag {args.lag} -> {tuple(poses.shape)}: {args.out}")
        return
    if isinstance(keypoints, list):
        poses = lift_tracks(model, keypoints, args.width, args.height, stride=args.stride, flip=not args.no_flip, max_windows=args.max_windows,
                            layout=args.layout)
        np.savez(args.out, **{f"track_{i}": final(p, keypoints[i], i).cpu().numpy() for i, p in enumerate(poses)}, **extras)
        print(f"lifted {len(keypoints)} tracks ({sum(len(k) for k in keypoints)} frames) -> {args.out}")
        return
    poses = final(lift_track(model, keypoints, args.width, args.height, stride=args.stride, flip=not args.no_flip, max_windows=args.max_windows,
                             layout=args.layout), keypoints)
    np.save(args.out, poses.cpu().numpy())
    print(f"lifted {keypoints.shape} -> {tuple(poses.shape)}: {args.out}")


if __name__ == "__main__":
    main()
