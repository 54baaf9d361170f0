#!/usr/bin/env python3
"""Constant limb lengths on the device (kasportsformer_amd.fix_bone_lengths / bone_lengths / BoneLengthFilter) against its neighbours and against what a caller
would do without it.

    python tools/bones_bench.py [--steps kernels live host] [--iters 50] [--reps 5] [--seed 0]

Every step runs in a child process of its own under its own time limit, one after the other; a step that fails or runs out of time ends the run.
  kernels  kasf_bone_median (two launches: lengths, select) and kasf_bone_apply alone, and as yardsticks kasf_pose_world and kasf_one_euro_tracks over the same
           poses in the same run, at three inputs: one 18,000-frame track, tools/lift_tracks_bench.py's `players` (22 tracks of 30-1,800 frames) and its `short`
           (200 tracks of 20-60 frames).  CUDA events around --iters back-to-back calls of the C entry, per call, the median of --reps; GB/s counts 204 B in and
           204 B out per frame for the apply and the yardsticks, 204 B in for the median.
  live     BoneLengthFilter.push at 22 and 1,024 rows, driven by slot ids and by a TrackResult; events, per call.
  host     the path fix_bone_lengths replaces, labelled as what it is: download + the numpy restatement (tests/bones_ref.py, whole arrays at once) + upload,
           host clock up to a synchronise, against the device call on the same clock; the two results are compared on their bits.
Prints one JSON line per measurement.  None of the numbers is a pass / fail bar.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kernels": 240, "live": 180, "host": 300}                # seconds per child
PRESETS = {"one_track": (1, 18000, 18000), "players": (22, 30, 1800), "short": (200, 20, 60)}     # tracks, shortest, longest (frames)
SLOTS = 32


def _events(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _input(np, name, seed):
    """Packed poses [N,17,3] of a moving figure with 2 cm of joint noise, and the offsets of the preset's tracks."""
    from tests.bones_ref import synthetic_track
    P, lo, hi = PRESETS[name]
    g = np.random.default_rng(seed)
    lengths = [int(n) for n in g.integers(lo, hi + 1, size=P)]
    off = np.cumsum([0] + lengths).astype(np.int64)
    return synthetic_track(int(off[-1]), 0.02, seed), off


def _track_arrays(np, streams, count):
    ids, slot = np.full((streams, SLOTS), -1, np.int32), np.zeros((streams, SLOTS), np.int32)
    ids[:, :count], slot[:, :count] = np.arange(1, count + 1), np.arange(count)
    return dict(ids=ids, slot=slot, born=np.zeros((streams, SLOTS), np.int32), count=np.full(streams, count, np.int32))


def step_kernels(args):
    import numpy as np
    import torch
    from kasportsformer_amd import _args, _lib
    from kasportsformer_amd.smooth import one_euro_params
    lib = _lib.load()
    for name in PRESETS:
        x_np, off = _input(np, name, args.seed)
        N, P = len(x_np), len(off) - 1
        x, offd, out = torch.from_numpy(x_np).cuda(), torch.from_numpy(off).cuda(), torch.empty((N, 17, 3), device="cuda")
        scratch, L = torch.empty(16 * N, device="cuda"), torch.empty((P, 16), device="cuda")
        cnt = torch.empty((P, 16), dtype=torch.int32, device="cuda")
        quat = (C.c_float * 4)(0.1407, -0.1500, -0.7552, 0.6223)
        euro = one_euro_params(min_score=0.0)
        s = _args.stream()
        calls = {
            "kasf_bone_median": (lambda: lib.kasf_bone_median(x.data_ptr(), offd.data_ptr(), N, P, scratch.data_ptr(), L.data_ptr(), cnt.data_ptr(), s), 204),
            "kasf_bone_apply": (lambda: lib.kasf_bone_apply(x.data_ptr(), offd.data_ptr(), N, P, L.data_ptr(), 1, 0, out.data_ptr(), s), 408),
            "kasf_pose_world": (lambda: lib.kasf_pose_world(x.data_ptr(), N, quat, None, 0, 0, out.data_ptr(), s), 408),
            "kasf_one_euro_tracks": (lambda: lib.kasf_one_euro_tracks(x.data_ptr(), offd.data_ptr(), N, P, 17, 3, 0, C.byref(euro), out.data_ptr(), s), 408),
        }
        ms = {}
        for what, (fn, bytes_per_frame) in calls.items():
            _lib.check(fn())
            ms[what] = statistics.median(_events(torch, fn, args.iters) for _ in range(args.reps))
            print(json.dumps({"what": what, "input": name, "tracks": P, "frames": N, "event_ms": round(ms[what], 5),
                              "GB_per_s": round(N * bytes_per_frame / ms[what] / 1e6, 1)}), flush=True)
        both = ms["kasf_bone_median"] + ms["kasf_bone_apply"]
        print(json.dumps({"what": "median + apply (fix_bone_lengths' three launches) against the yardsticks", "input": name, "event_ms": round(both, 5),
                          "over_pose_world": round(both / ms["kasf_pose_world"], 2), "over_one_euro_tracks": round(both / ms["kasf_one_euro_tracks"], 3),
                          "apply_over_pose_world": round(ms["kasf_bone_apply"] / ms["kasf_pose_world"], 2), "device": torch.cuda.get_device_name(0)}), flush=True)


def step_live(args):
    import numpy as np
    import torch
    from types import SimpleNamespace
    import kasportsformer_amd as K
    from tests.bones_ref import synthetic_track
    for rows in (22, 1024):
        x = torch.from_numpy(synthetic_track(rows, 0.02, rows)).cuda()
        f = K.BoneLengthFilter(slots=rows)
        f.push(x)
        ms = statistics.median(_events(torch, lambda: f.push(x), args.iters) for _ in range(args.reps))
        print(json.dumps({"what": "BoneLengthFilter.push (kasf_bone_push), per call", "rows": rows, "event_ms": round(ms, 5)}), flush=True)
        streams, mode, R = (1, "persons", 22) if rows == 22 else (32, "tracks", 32)
        t = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in _track_arrays(np, streams, R).items()})
        ft = K.BoneLengthFilter(streams=streams, track_slots=SLOTS, rows=mode, num_person=R)
        ft.push(x, t)
        ms = statistics.median(_events(torch, lambda: ft.push(x, t), args.iters) for _ in range(args.reps))
        print(json.dumps({"what": "BoneLengthFilter.push(poses, TrackResult) (kasf_bone_tracked), per call", "rows": rows, "streams": streams,
                          "event_ms": round(ms, 5)}), flush=True)


def step_host(args):
    import numpy as np
    import torch
    import kasportsformer_amd as K
    from tests.bones_ref import apply_arrays_np, median_np

    def host_path(x, off):
        a = x.cpu().numpy()
        L, _ = median_np(a, off)
        return torch.from_numpy(apply_arrays_np(a, off, L, False)).cuda()
    for name in PRESETS:
        x_np, off = _input(np, name, args.seed)
        x = torch.from_numpy(x_np).cuda()
        K.fix_bone_lengths(x, off)
        d, e_d = _wall(torch, lambda: K.fix_bone_lengths(x, off))
        h, e_h = _wall(torch, lambda: host_path(x, off))
        print(json.dumps({"what": "fix_bone_lengths vs download + the numpy restatement + upload, host clock", "input": name, "frames": len(x_np),
                          "device_wall_ms": round(e_d, 4), "host_path_wall_ms": round(e_h, 2),
                          "bits_equal": bool(np.array_equal(d.cpu().numpy().view(np.uint32), h.cpu().numpy().view(np.uint32)))}), flush=True)


STEPS = {"kernels": step_kernels, "live": step_live, "host": step_host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", choices=list(STEPS), default=list(STEPS))
    ap.add_argument("--child", choices=list(STEPS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.child is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("bones_bench: needs a GPU; there is no CPU path to time")
        STEPS[args.child](args)
        return
    passed = [a for a in sys.argv[1:]]
    for step in args.steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step] + passed, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            sys.exit(f"bones_bench: step {step} did not finish in {LIMITS[step]} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"bones_bench: step {step} ended with status {r.returncode}; nothing further is started")


if __name__ == "__main__":
    main()
