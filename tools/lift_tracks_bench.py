#!/usr/bin/env python3
"""Many 2-D tracks of different lengths: one kasportsformer_amd.lift_tracks call against a loop of lift_track, one call per track.

    python tools/lift_tracks_bench.py --preset players|short [--layers 26] [--dtype bf16] [--reps 5] [--kernel-iters 20] [--seed 0]

The shipped model (26 layers, 8 heads, T = 27, bf16; random weights, which the time does not depend on) and a seeded track set:
  players  22 tracks of 30-1,800 frames (broadcast football: every player in view gets a track, players enter and leave)
  short    200 tracks of 20-60 frames (many brief tracks: each is one or two windows, so the loop runs 200 small-batch forwards)
The tracks are on the device before timing; flip-TTA on, the demo's windows (stride T), max_windows at its default.  Both ways are timed with
CUDA events around the whole call, closed by a synchronise, the two alternating within each rep; the median over --reps after one warm-up of
each.  kasf_lift_windows_ragged and kasf_lift_stitch_ragged are timed alone on the same plan: events around --kernel-iters back-to-back launches,
per launch.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kasportsformer_amd as K  # noqa: E402
from kasportsformer_amd import _lib  # noqa: E402
from kasportsformer_amd._args import stream  # noqa: E402
from kasportsformer_amd.lift import ragged_plan  # noqa: E402

PRESETS = {"players": (22, 30, 1800), "short": (200, 20, 60)}     # tracks, shortest, longest (frames)


def _timed(fn):
    """(CUDA-event ms, host wall ms) of fn() up to a synchronise after it."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="players")
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    T, W_PX, H_PX = 27, 1280, 720
    P, lo, hi = PRESETS[args.preset]
    g = np.random.default_rng(args.seed)
    lengths = [int(n) for n in g.integers(lo, hi + 1, size=P)]
    tracks = [torch.from_numpy(np.concatenate((g.uniform((0, 0), (W_PX, H_PX), size=(n, 17, 2)), g.uniform(0.3, 1, size=(n, 17, 1))),
                                              axis=-1).astype(np.float32)).cuda() for n in lengths]
    model = K.KASportsFormer(n_layers=args.layers, num_heads=8, n_frames=T, compute_dtype=args.dtype).cuda().eval()

    def loop():
        return [K.lift_track(model, t, W_PX, H_PX) for t in tracks]

    def batched():
        return K.lift_tracks(model, tracks, W_PX, H_PX)

    ref, got = loop(), batched()                                     # warm-up: weight packing, the workspace of every batch size
    max_diff = max(float((a - b).abs().max()) for a, b in zip(ref, got))
    ms, wall = {"loop": [], "lift_tracks": []}, {"loop": [], "lift_tracks": []}
    for _ in range(args.reps):
        for name, fn in (("loop", loop), ("lift_tracks", batched)):
            e, w = _timed(fn)
            ms[name].append(e)
            wall[name].append(w)

    lib = _lib.load()
    win_first, r, fp = ragged_plan(lengths, T, T)
    off = np.cumsum([0] + lengths, dtype=np.int64)
    frames, windows = int(off[-1]), int(win_first[-1])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    off_d, wf_d, r_d, fp_d = dev(off), dev(win_first), dev(r), dev(fp)
    w_d, h_d = dev(np.full(P, W_PX, np.float32)), dev(np.full(P, H_PX, np.float32))
    packed = torch.cat(tracks)
    x = torch.empty((2 * windows, T, 17, 3), device="cuda")
    pred = torch.randn_like(x)
    poses = torch.empty((frames, 17, 3), device="cuda")
    launches = {
        "windows_ragged": lambda: lib.kasf_lift_windows_ragged(packed.data_ptr(), off_d.data_ptr(), wf_d.data_ptr(), P, frames, windows, w_d.data_ptr(),
                                                               h_d.data_ptr(), T, T, r_d.data_ptr(), 1, x.data_ptr(), stream()),
        "stitch_ragged": lambda: lib.kasf_lift_stitch_ragged(pred.data_ptr(), 1, off_d.data_ptr(), wf_d.data_ptr(), P, frames, windows, T, T,
                                                             fp_d.data_ptr(), poses.data_ptr(), stream()),
    }
    for name, launch in launches.items():
        _lib.check(launch())
        ms[name] = []
        for _ in range(args.reps):
            e, _ = _timed(lambda: [_lib.check(launch()) for _ in range(args.kernel_iters)])
            ms[name].append(e / args.kernel_iters)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"what": "many tracks: one lift_tracks call vs a lift_track loop (measured, CUDA events, median of %d)" % args.reps,
                      "preset": args.preset, "tracks": P, "frames": frames, "frames_min": min(lengths), "frames_max": max(lengths),
                      "windows": windows, "clips": 2 * windows, "layers": args.layers, "dtype": args.dtype,
                      "forwards": {"loop": P, "lift_tracks": math.ceil(windows / 1024)},
                      "ms": {k: round(v, 4) for k, v in med.items()}, "speedup": round(med["loop"] / med["lift_tracks"], 2),
                      "wall_ms": {k: round(statistics.median(v), 3) for k, v in wall.items()},
                      "ms_all_reps": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
                      "max_abs_diff_loop_vs_lift_tracks": max_diff, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
