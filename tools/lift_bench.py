#!/usr/bin/env python3
"""Phase timing of lifting one long 2-D track (kasportsformer_amd.lift_track's three stages, run here one by one).

    python tools/lift_bench.py [--frames 18000] [--layers 26] [--dtype bf16] [--reps 5]

The shipped model (26 layers, 8 heads, T = 27, bf16), one person, an 18,000-frame track (10 minutes at 30 fps): 667 windows, 1,334 clips
with flip-TTA.  kasf_lift_windows, the forward of the stacked batch and kasf_lift_stitch are timed separately with CUDA events on the current
stream (median over --reps after one warm-up lift), and the whole lift_track call end to end.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kasportsformer_amd as K  # noqa: E402
from kasportsformer_amd import _lib  # noqa: E402
from kasportsformer_amd._args import stream  # noqa: E402
from kasportsformer_amd.lift import window_plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=18000)
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    T, W_PX, H_PX = 27, 1280, 720
    model = K.KASportsFormer(n_layers=args.layers, num_heads=8, n_frames=T, compute_dtype=args.dtype).cuda().eval()
    g = np.random.default_rng(0)
    n = args.frames
    kp = np.concatenate((g.uniform((0, 0), (W_PX, H_PX), size=(n, 17, 2)), g.uniform(0.3, 1, size=(n, 17, 1))), axis=-1).astype(np.float32)
    track = torch.from_numpy(kp).cuda()
    lib = _lib.load()
    starts, _, r, fp = window_plan(n, T)
    W = len(starts)
    r_dev = torch.from_numpy(r).cuda() if r is not None else None
    fp_dev = torch.from_numpy(fp).cuda() if fp is not None else None
    x = torch.empty((2 * W, T, 17, 3), device="cuda")
    poses = torch.empty((1, n, 17, 3), device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    phases = {"windows": [], "forward": [], "stitch": [], "lift_track": []}
    K.lift_track(model, track, W_PX, H_PX)                     # warm-up: weight packing, workspace allocation
    torch.cuda.synchronize()
    with torch.no_grad():
        for _ in range(args.reps):
            ev[0].record()
            _lib.check(lib.kasf_lift_windows(track.data_ptr(), 1, n, float(W_PX), float(H_PX), T, T, r_dev.data_ptr() if r_dev is not None else None, 1,
                                             x.data_ptr(), stream()))
            ev[1].record()
            pred = model(x)
            ev[2].record()
            _lib.check(lib.kasf_lift_stitch(pred.data_ptr(), 1, 1, n, T, T, fp_dev.data_ptr() if fp_dev is not None else None, poses.data_ptr(), stream()))
            ev[3].record()
            K.lift_track(model, track, W_PX, H_PX)
            ev[4].record()
            torch.cuda.synchronize()
            for k, name in enumerate(phases):
                phases[name].append(ev[k].elapsed_time(ev[k + 1]))
    ms = {k: statistics.median(v) for k, v in phases.items()}
    print(json.dumps({"what": "lift of one 2-D track (measured, CUDA events, median of %d)" % args.reps, "frames": n, "T": T, "windows": W, "clips": 2 * W,
                      "layers": args.layers, "dtype": args.dtype, "ms": {k: round(v, 4) for k, v in ms.items()},
                      "ms_all_reps": {k: [round(x, 4) for x in v] for k, v in phases.items()},
                      "windows_per_s": round(W / (ms["lift_track"] / 1e3), 1), "clips_per_s_forward": round(2 * W / (ms["forward"] / 1e3), 1),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
