"""Lifting a 2-D keypoint track to 3-D poses on the GPU: the demo's stage 2 (demo/demo.py:194-254, ``lift_3d_pose``) without the detectors.

    poses = lift_track(model, keypoints, width, height)          # keypoints [N,17,3] or [P,N,17,3] pixels + confidence -> [..., 17, 3]

The demo cuts the track into T-frame clips (``turn_into_clips`` / ``resample``, demo.py:132-156), normalises them
(``normalize_screen_coordinates``, demo/lib/utils.py:16-20), runs two forwards per clip (plain and ``flip_data``-mirrored), averages the
flip-TTA pair, zeroes the root and keeps the original frames of the resampled tail clip.  Here one kernel cuts, normalises and mirrors
every window of every person (``kasf_lift_windows``), the forward runs on stacked batches of windows, and one kernel merges the pair and
puts the frames back on the track (``kasf_lift_stitch``).  Two demo bugs are not reproduced: ``flip_data`` flips its argument in place
(demo.py:227: both forwards see the mirrored clip), and ``turn_into_clips`` raises ``UnboundLocalError`` when N > T and N % T == 0.

``stride < T`` selects overlapping windows (not in the demo): each frame is the mean over the windows that cover it.

    python -m kasportsformer_amd.lift --config X.yaml --checkpoint best.pth --keypoints keypoints2d.pkl --width 1280 --height 720 --out poses3d.npy
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import pickle

import numpy as np
import torch

from . import _lib


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


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _model_device(model) -> torch.device:
    dev = model._flat.device
    if dev.type != "cuda":
        raise RuntimeError("lift_track: the model must be on the GPU (model.cuda()); kasportsformer_amd has no CPU path")
    return dev


def _track(keypoints, device) -> torch.Tensor:
    if isinstance(keypoints, np.ndarray):
        if keypoints.dtype != np.float32:
            raise TypeError(f"lift_track: keypoints must be float32, got {keypoints.dtype}")
        kp = torch.from_numpy(np.ascontiguousarray(keypoints))
    elif isinstance(keypoints, torch.Tensor):
        if keypoints.dtype != torch.float32:
            raise TypeError(f"lift_track: keypoints must be float32, got {keypoints.dtype}")
        if keypoints.is_cuda and keypoints.device != device:
            raise RuntimeError(f"lift_track: keypoints are on {keypoints.device}, the model on {device}")
        if not keypoints.is_cuda and keypoints.device.type != "cpu":
            raise RuntimeError(f"lift_track: keypoints on unsupported device {keypoints.device}")
        kp = keypoints.detach()
    else:
        raise TypeError(f"lift_track: keypoints must be a numpy array or a torch tensor, got {type(keypoints).__name__}")
    if kp.dim() not in (3, 4) or tuple(kp.shape[-2:]) != (17, 3):
        raise ValueError(f"lift_track: expected keypoints [N,17,3] or [P,N,17,3], got {tuple(kp.shape)}")
    return kp.to(device).contiguous()            # a copy when it comes from the host; on the device the kernels only read it


def lift_track(model, keypoints, width, height, *, stride=None, flip: bool = True, max_windows: int = 1024) -> torch.Tensor:
    """3-D poses of a 2-D keypoint track: ``keypoints`` [N,17,3] or [P,N,17,3] float32 (pixel x, y, confidence; numpy or torch, CPU or
    GPU, never modified) -> CUDA fp32 [N,17,3] / [P,N,17,3] in the model's output space with the root joint at zero (the demo's
    ``output_3D`` before ``camera_to_world``).  T is ``model.n_frames``; ``stride`` defaults to T (the demo's clips).  The forward runs in
    eval mode without autograd, the plain and mirrored views of each window in one stacked batch, at most ``max_windows`` windows
    (2 * ``max_windows`` clips with ``flip``) per call; ``model.training`` is restored afterwards."""
    device = _model_device(model)
    kp = _track(keypoints, device)
    lead = tuple(kp.shape[:-2])
    kp4 = kp if kp.dim() == 4 else kp.unsqueeze(0)
    P, n = int(kp4.shape[0]), int(kp4.shape[1])
    T = int(model.n_frames)
    stride = T if stride is None else int(stride)
    if not 1 <= stride <= T:
        raise ValueError(f"lift_track: stride must be in [1, T={T}], got {stride}")
    if int(max_windows) < 1:
        raise ValueError("lift_track: max_windows must be >= 1")
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
        x = torch.empty((halves * PW, T, 17, 3), dtype=torch.float32, device=device)
        _lib.check(lib.kasf_lift_windows(kp4.data_ptr(), P, n, float(width), float(height), T, stride,
                                         r_dev.data_ptr() if r_dev is not None else None, int(flip), x.data_ptr(), _stream()))
        was_training = model.training
        model.eval()
        try:
            if PW <= max_windows:
                pred = model(x)                                      # the whole lift in one stacked batch
            else:
                pred = torch.empty_like(x)
                for a in range(0, PW, max_windows):
                    b = min(a + max_windows, PW)
                    idx = [slice(h * PW + a, h * PW + b) for h in range(halves)]
                    out = model(torch.cat([x[i] for i in idx]) if flip else x[idx[0]])
                    for h, i in enumerate(idx):
                        pred[i].copy_(out[h * (b - a):(h + 1) * (b - a)])
        finally:
            model.train(was_training)
        poses = torch.empty((P, n, 17, 3), dtype=torch.float32, device=device)
        _lib.check(lib.kasf_lift_stitch(pred.data_ptr(), int(flip), P, n, T, stride, fp_dev.data_ptr() if fp_dev is not None else None,
                                        poses.data_ptr(), _stream()))
    return poses.view(lead + (17, 3))


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


def load_keypoints(path: str) -> np.ndarray:
    """[P,N,17,3] (or [N,17,3]) float32 keypoints from a ``.npy`` file (no pickles) or a ``.pkl`` file of numpy arrays only."""
    if str(path).endswith(".npy"):
        kp = np.load(path, allow_pickle=False)
    else:
        with open(path, "rb") as f:
            kp = _KeypointUnpickler(io.BytesIO(f.read())).load()
    if not isinstance(kp, np.ndarray) or kp.dtype.hasobject:
        raise TypeError(f"{path}: expected a numeric numpy array, got {type(kp).__name__} {getattr(kp, 'dtype', '')}")
    return np.ascontiguousarray(kp, dtype=np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m kasportsformer_amd.lift", description="Lift a 2-D keypoint track to 3-D poses (demo.py stage 2).")
    ap.add_argument("--config", required=True, help="model yaml (configs/*.yaml)")
    ap.add_argument("--checkpoint", required=True, help="checkpoint written by checkpoint_save or the reference's training script")
    ap.add_argument("--keypoints", required=True, help="keypoints2d.pkl ([P,N,17,3], the demo's detect_2d_pose output) or .npy")
    ap.add_argument("--width", type=float, required=True, help="frame width in pixels")
    ap.add_argument("--height", type=float, required=True, help="frame height in pixels")
    ap.add_argument("--stride", type=int, default=None, help="window stride (default: T, the demo's clips; < T: overlapping windows averaged)")
    ap.add_argument("--no-flip", action="store_true", help="skip the flip-TTA pair")
    ap.add_argument("--compute-dtype", choices=("bf16", "fp32"), default=None, help="default: the yaml's compute_dtype, else bf16")
    ap.add_argument("--max-windows", type=int, default=1024)
    ap.add_argument("--out", required=True, help="output .npy of [P,N,17,3] (or [N,17,3]) float32 poses")
    args = ap.parse_args(argv)

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
    poses = lift_track(model, keypoints, args.width, args.height, stride=args.stride, flip=not args.no_flip, max_windows=args.max_windows)
    np.save(args.out, poses.cpu().numpy())
    print(f"lifted {keypoints.shape} -> {tuple(poses.shape)}: {args.out}")


if __name__ == "__main__":
    main()
