#!/usr/bin/env python3
"""COCO detector keypoints in, world-space poses out: ``layout="coco"`` against what a caller did before it existed, the two new kernels alone, and
the live-stream tick with and without the conversion.

    python tools/coco_bench.py [--layers 26] [--dtype bf16] [--reps 5] [--kernel-iters 20] [--ticks 200] [--warmup 40] [--seed 0]

The shipped model (26 layers, 8 heads, T = 27, bf16; random weights, which the time does not depend on), flip-TTA on, 1280 x 720, seeded COCO-17 keypoints:
  track    one 18,000-frame track (ten minutes of one player at 30 fps) through lift_track
  players  lift_tracks_bench.py's ``players`` preset (22 tracks of 30-1,800 frames) through lift_tracks
For both, from keypoints in host memory: (a) ``layout="coco"`` -- upload, convert on the device, lift -- against (b) today's way -- the reference's
numpy conversion on the host (tests/test_coco_world_cpu.py's restatement of h36m_coco_format, bit-equal to it), upload, the default layout; (c) is (a)
with the keypoints already on the device.  CUDA events and the host clock around each, median of --reps; the poses of (a) and (b) are compared.
Kernels alone, events around --kernel-iters back-to-back launches, per launch, with achieved GB/s (bytes read + written): kasf_coco_h36m and
kasf_pose_world (floor + unit) on the 18,000 frames and on 1,000,000, and kasf_lift_windows (flip) on the same frames as the yardstick.
Stream: 22 slots, lag 0, frames on the device; StreamLifter.push per tick with and without ``layout="coco"``, alternating within the tick, median and
99th percentile of --ticks ticks after --warmup.  Prints one JSON line.
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
from kasportsformer_amd.lift import window_plan  # noqa: E402
from tests.test_coco_world_cpu import coco_h36m_np  # noqa: E402

PLAYERS = (22, 30, 1800)                # lift_tracks_bench.py's preset: tracks, shortest, longest (frames)
T, W_PX, H_PX = 27, 1280, 720


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


def _coco(g, n):
    return np.concatenate((g.uniform((0, 0), (W_PX, H_PX), size=(n, 17, 2)), g.uniform(0.3, 1, size=(n, 17, 1))), axis=-1).astype(np.float32)


def _compare(ways, reps):
    """{name: fn} -> event / wall medians per way, alternating the ways within a repetition, after one warm-up call of each."""
    first = {k: fn() for k, fn in ways.items()}
    ms, wall = {k: [] for k in ways}, {k: [] for k in ways}
    for _ in range(reps):
        for k, fn in ways.items():
            _, e, w = _timed(fn)
            ms[k].append(e)
            wall[k].append(w)
    return first, {"event_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()}, "wall_ms": {k: round(statistics.median(v), 4) for k, v in wall.items()}}


def _stats(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "p99": round(v[min(len(v) - 1, int(0.99 * len(v)))], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    g = np.random.default_rng(args.seed)
    model = K.KASportsFormer(n_layers=args.layers, num_heads=8, n_frames=T, compute_dtype=args.dtype).cuda().eval()
    res = {"what": "COCO keypoints in, world poses out (measured; CUDA events and host clock, median of %d)" % args.reps,
           "layers": args.layers, "dtype": args.dtype, "T": T, "device": torch.cuda.get_device_name(0)}

    # one long track
    track = _coco(g, 18000)
    track_d = torch.from_numpy(track).cuda()
    first, t = _compare({"layout_coco": lambda: K.lift_track(model, track, W_PX, H_PX, layout="coco"),
                         "host_numpy_then_default": lambda: K.lift_track(model, coco_h36m_np(track), W_PX, H_PX),
                         "layout_coco_device_input": lambda: K.lift_track(model, track_d, W_PX, H_PX, layout="coco")}, args.reps)
    t0 = time.perf_counter()
    coco_h36m_np(track)
    t["host_numpy_conversion_alone_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
    t["max_abs_diff"] = float((first["layout_coco"] - first["host_numpy_then_default"]).abs().max())
    res["track_18000"] = t

    # many tracks
    P, lo, hi = PLAYERS
    lengths = [int(n) for n in g.integers(lo, hi + 1, size=P)]
    tracks = [_coco(g, n) for n in lengths]
    tracks_d = [torch.from_numpy(a).cuda() for a in tracks]
    first, t = _compare({"layout_coco": lambda: K.lift_tracks(model, tracks, W_PX, H_PX, layout="coco"),
                         "host_numpy_then_default": lambda: K.lift_tracks(model, [coco_h36m_np(a) for a in tracks], W_PX, H_PX),
                         "layout_coco_device_input": lambda: K.lift_tracks(model, tracks_d, W_PX, H_PX, layout="coco")}, args.reps)
    t["max_abs_diff"] = max(float((a - b).abs().max()) for a, b in zip(first["layout_coco"], first["host_numpy_then_default"]))
    t.update(tracks=P, frames=sum(lengths))
    res["players"] = t

    # the kernels alone
    lib = _lib.load()
    q = np.asarray(K.DEMO_CAMERA_ROTATION, np.float32)
    kernels = {}
    for frames in (18000, 1000000):
        src = torch.from_numpy(_coco(g, frames)).cuda()
        dst = torch.empty_like(src)
        x = torch.empty((2 * len(window_plan(frames, T)[0]), T, 17, 3), device="cuda")
        r = window_plan(frames, T)[2]
        r_d = torch.from_numpy(r).cuda() if r is not None else None
        launches = {
            "coco_h36m": (408, lambda: lib.kasf_coco_h36m(src.data_ptr(), frames, dst.data_ptr(), stream())),
            "pose_world_floor_unit": (408, lambda: lib.kasf_pose_world(src.data_ptr(), frames, q.ctypes.data, None, 1, 1, dst.data_ptr(), stream())),
            "lift_windows_flip (yardstick)": (612, lambda: lib.kasf_lift_windows(src.data_ptr(), 1, frames, float(W_PX), float(H_PX), T, T,
                                                                               r_d.data_ptr() if r_d is not None else None, 1, x.data_ptr(), stream())),
        }
        for name, (bytes_per_frame, launch) in launches.items():
            _lib.check(launch())
            reps = []
            for _ in range(args.reps):
                _, e, _ = _timed(lambda: [_lib.check(launch()) for _ in range(args.kernel_iters)])
                reps.append(e / args.kernel_iters)
            ms = statistics.median(reps)
            kernels[f"{name} @ {frames}"] = {"ms": round(ms, 5), "GB_per_s": round(bytes_per_frame * frames / ms / 1e6, 1)}
        del src, dst, x
    res["kernels"] = kernels

    # the live tick
    S, n = 22, args.warmup + args.ticks
    ticks = torch.from_numpy(_coco(g, n * S).reshape(n, S, 17, 3)).cuda()
    with_coco, without = K.StreamLifter(model, W_PX, H_PX, slots=S, layout="coco"), K.StreamLifter(model, W_PX, H_PX, slots=S)
    ms = {"push_layout_coco": [], "push_default": []}
    for i in range(n):
        _, e_a, _ = _timed(lambda: with_coco.push(ticks[i]))
        _, e_b, _ = _timed(lambda: without.push(ticks[i]))
        if i >= args.warmup:
            ms["push_layout_coco"].append(e_a)
            ms["push_default"].append(e_b)
    res["stream_22_slots_event_ms"] = {k: _stats(v) for k, v in ms.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
