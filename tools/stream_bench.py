#!/usr/bin/env python3
"""Live keypoint streams: one kasportsformer_amd.StreamLifter.push per tick against what a caller did before it existed, lift_tracks on every
player's last T frames with the last pose taken.

    python tools/stream_bench.py --preset players|one [--layers 26] [--dtype bf16] [--ticks 200] [--warmup 40] [--kernel-iters 20] [--seed 0]

The shipped model (26 layers, 8 heads, T = 27, bf16; random weights, which the time does not depend on), flip-TTA on, lag 0, seeded keypoints that
are on the device before timing:
  players  22 slots (broadcast football: every player in view)
  one      1 slot
After --warmup ticks of both ways (the rings are full from tick T on), --ticks ticks, each running (a) lifter.push(frame) and (b) lift_tracks on
the [T,17,3] histories of all slots, poses[-1] of each, alternating within the tick; each timed with CUDA events and with the host clock up to a
synchronise.  Reports median and 99th percentile per tick of both, the largest difference between their poses, and kasf_stream_push / _windows /
_emit alone: events around --kernel-iters back-to-back launches, per launch.  Prints one JSON line.
"""
import argparse
import json
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

PRESETS = {"players": 22, "one": 1}     # slots


def _timed(fn):
    """(result, CUDA-event ms, host wall ms) of fn() up to a synchronise after it."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def _stats(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "p99": round(v[min(len(v) - 1, int(0.99 * len(v)))], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=sorted(PRESETS), default="players")
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5, help="repetitions of the kernel-alone timings")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    T, W_PX, H_PX = 27, 1280, 720
    S = PRESETS[args.preset]
    if args.warmup < T:
        ap.error(f"--warmup must be at least T = {T}: both ways are timed on full windows")
    n = args.warmup + args.ticks
    g = np.random.default_rng(args.seed)
    stream_kp = torch.from_numpy(np.concatenate((g.uniform((0, 0), (W_PX, H_PX), size=(n, S, 17, 2)), g.uniform(0.3, 1, size=(n, S, 17, 1))),
                                                axis=-1).astype(np.float32)).cuda()           # [ticks, slots, 17, 3]
    by_slot = stream_kp.transpose(0, 1).contiguous()                                          # [slots, ticks, 17, 3]: the caller's own history buffers
    model = K.KASportsFormer(n_layers=args.layers, num_heads=8, n_frames=T, compute_dtype=args.dtype).cuda().eval()
    lifter = K.StreamLifter(model, W_PX, H_PX, slots=S, flip=True, lag=0)

    def online(t):
        return lifter.push(stream_kp[t])

    def today(t):
        a = max(0, t + 1 - T)
        return torch.stack([p[-1] for p in K.lift_tracks(model, [by_slot[s, a:t + 1] for s in range(S)], W_PX, H_PX)])

    ms, wall = {"push": [], "lift_tracks": []}, {"push": [], "lift_tracks": []}
    max_diff = 0.0
    for t in range(n):
        got, e_a, w_a = _timed(lambda: online(t))
        ref, e_b, w_b = _timed(lambda: today(t))
        max_diff = max(max_diff, float((got - ref).abs().max()))
        if t >= args.warmup:
            ms["push"].append(e_a)
            wall["push"].append(w_a)
            ms["lift_tracks"].append(e_b)
            wall["lift_tracks"].append(w_b)

    lib = _lib.load()
    frame = stream_kp[0]
    x = torch.empty((2 * S, T, 17, 3), device="cuda")
    pred = torch.randn_like(x)
    out = torch.empty((S, 1, 17, 3), device="cuda")
    ring, count = lifter._ring.clone(), lifter._count.clone()
    launches = {
        "stream_push": lambda: lib.kasf_stream_push(frame.data_ptr(), None, S, S, T, ring.data_ptr(), count.data_ptr(), stream()),
        "stream_windows": lambda: lib.kasf_stream_windows(ring.data_ptr(), count.data_ptr(), None, S, S, T, lifter._width.data_ptr(),
                                                          lifter._height.data_ptr(), lifter._r_tab.data_ptr(), 1, x.data_ptr(), stream()),
        "stream_emit": lambda: lib.kasf_stream_emit(pred.data_ptr(), 1, count.data_ptr(), None, S, S, T, lifter._fp_tab.data_ptr(), 0, 1,
                                                    out.data_ptr(), stream()),
    }
    kernel_ms = {}
    for name, launch in launches.items():
        _lib.check(launch())
        reps = []
        for _ in range(args.reps):
            _, e, _ = _timed(lambda: [_lib.check(launch()) for _ in range(args.kernel_iters)])
            reps.append(e / args.kernel_iters)
        kernel_ms[name] = round(statistics.median(reps), 5)
    print(json.dumps({"what": "live streams: StreamLifter.push per tick vs lift_tracks on every slot's last T frames (measured, %d ticks after %d warm-up)"
                              % (args.ticks, args.warmup),
                      "preset": args.preset, "slots": S, "clips_per_tick": 2 * S, "T": T, "layers": args.layers, "dtype": args.dtype, "lag": 0,
                      "event_ms": {k: _stats(v) for k, v in ms.items()}, "wall_ms": {k: _stats(v) for k, v in wall.items()},
                      "wall_median_ratio_lift_tracks_over_push": round(statistics.median(wall["lift_tracks"]) / statistics.median(wall["push"]), 3),
                      "kernel_ms_per_launch": kernel_ms, "max_abs_diff_push_vs_lift_tracks": max_diff,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
