#!/usr/bin/env python3
"""The recorded-track refinement on the device (kasportsformer_amd.refine_tracks, kasf_tracks_refine) next to the stages it stands beside and the host path it
replaces.

    python tools/refine_bench.py [--steps launches host] [--iters 20] [--reps 5] [--seed 0]

Every step runs in a child process of its own under its own `timeout -k 10`, one after the other; a step that fails or runs out of time ends the run.
  launches  kasf_tracks_refine alone (defaults: sigma 2, radius 6, max_gap 15; and the widest window, radius 32 with max_gap 64) over keypoints 17 x (x, y,
            score) with about 11 % of the joints gated in runs of 1 - 10 frames: one 18,000-frame track, and tools/lift_tracks_bench.py's `players` (22 tracks
            of 30 - 1,800 frames) and `short` (200 tracks of 20 - 60 frames).  CUDA events around --iters back-to-back calls of the C entry, per call, the
            median of --reps; GB/s of the bytes read + written (x, out, state).  In the same run, over the same rows, kasf_one_euro_tracks (the causal filter)
            and kasf_pose_world (a pure streaming kernel over 17 x 3 rows) as yardsticks.
  host      the path it replaces for the same inputs: download of the keypoints, the numpy restatement of the rule (tests/refine_ref.py), upload of the
            result; host clock up to a synchronise; its result is compared with the device's on its bits.
Prints one JSON line per measurement.  None of the numbers is a pass / fail bar.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"launches": 180, "host": 300}                            # seconds per child
J = 17
PRESETS = {"one": (1, 18000, 18000), "players": (22, 30, 1800), "short": (200, 20, 60)}      # tracks, shortest, longest (frames)


def _events(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _tracks(np, preset, seed):
    """(x [N, 17, 3] fp32 packed, offsets int64 [P + 1]): pixel positions, scores in [0.5, 1), about 11 % of the joints in runs of 1 - 10 frames scored below 0.3."""
    P, lo, hi = PRESETS[preset]
    g = np.random.default_rng(seed)
    off = np.cumsum([0] + [int(n) for n in g.integers(lo, hi + 1, size=P)]).astype(np.int64)
    N = int(off[-1])
    x = np.concatenate((g.uniform(0, 1000, (N, J, 2)), g.uniform(0.5, 1, (N, J, 1))), -1).astype(np.float32)
    starts = g.random((N, J)) < 0.11 / 5.5
    for f, j in zip(*np.nonzero(starts)):
        x[f:f + int(g.integers(1, 11)), j, 2] = 0.1
    return x, off


def _refine_call(torch, C, lib, _lib, stream, xd, od, out, state, q):
    N, P = xd.shape[0], od.shape[0] - 1
    return lambda: _lib.check(lib.kasf_tracks_refine(xd.data_ptr(), od.data_ptr(), N, P, J, 2, 1, C.byref(q), out.data_ptr(), state.data_ptr(), stream()))


def step_launches(args):
    import ctypes as C
    import numpy as np
    import torch
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import stream
    from kasportsformer_amd.pose import DEMO_CAMERA_ROTATION
    from kasportsformer_amd.refine import refine_params
    from kasportsformer_amd.smooth import one_euro_params
    lib = _lib.load()
    for preset in PRESETS:
        x, off = _tracks(np, preset, args.seed)
        N, P = x.shape[0], len(off) - 1
        xd, od = torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda()
        out, state = torch.empty_like(xd), torch.empty((N, J), dtype=torch.uint8, device="cuda")
        moved = 2 * x.nbytes + N * J

        def report(what, fn, nbytes, **kw):
            fn()
            ms = statistics.median(_events(torch, fn, args.iters) for _ in range(args.reps))
            print(json.dumps({"what": what, "preset": preset, "tracks": P, "frames": N, "event_ms": round(ms, 5), "GBps": round(nbytes / ms / 1e6, 2), **kw}),
                  flush=True)
        for name, q in (("defaults (sigma 2, radius 6, max_gap 15)", refine_params()), ("widest (sigma 11, radius 32, max_gap 64)", refine_params(0.3, 64, 11.0, 32))):
            report(f"kasf_tracks_refine, {name}", _refine_call(torch, C, lib, _lib, stream, xd, od, out, state, q), moved)
        pe = one_euro_params()
        report("kasf_one_euro_tracks (yardstick: the causal filter over the same rows)",
               lambda: _lib.check(lib.kasf_one_euro_tracks(xd.data_ptr(), od.data_ptr(), N, P, J, 2, 1, C.byref(pe), out.data_ptr(), stream())), 2 * x.nbytes)
        q4 = np.asarray(DEMO_CAMERA_ROTATION, np.float32)
        t3 = np.zeros(3, np.float32)
        report("kasf_pose_world (yardstick: a streaming kernel over the same rows as 17 x 3 poses)",
               lambda: _lib.check(lib.kasf_pose_world(xd.data_ptr(), N, q4.ctypes.data, t3.ctypes.data, 0, 0, out.data_ptr(), stream())), 2 * x.nbytes,
               device=torch.cuda.get_device_name(0))


def step_host(args):
    import numpy as np
    import torch
    import kasportsformer_amd as K
    from tests.refine_ref import refine_np, weights
    w, radius = weights(2.0)
    for preset in PRESETS:
        x, off = _tracks(np, preset, args.seed)
        xd = torch.from_numpy(x).cuda()
        K.refine_tracks(xd, offsets=off)
        wall = {}
        for name, fn in (("device", lambda: K.refine_tracks(xd, offsets=off)),
                         ("host", lambda: torch.from_numpy(refine_np(xd.cpu().numpy(), off, True, 0.3, 15, w, radius)[0]).cuda())):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            wall[name] = ((time.perf_counter() - t0) * 1e3, got.cpu().numpy().view(np.uint32))
        print(json.dumps({"what": "refine_tracks vs download + numpy restatement + upload, host clock", "preset": preset, "tracks": len(off) - 1,
                          "frames": int(off[-1]), "device_wall_ms": round(wall["device"][0], 4), "host_path_wall_ms": round(wall["host"][0], 2),
                          "bits_equal": bool(np.array_equal(wall["device"][1], wall["host"][1]))}), flush=True)


STEPS = {"launches": step_launches, "host": step_host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", choices=list(STEPS), default=list(STEPS))
    ap.add_argument("--child", choices=list(STEPS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.child is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("refine_bench: needs a GPU; there is no CPU path to time")
        STEPS[args.child](args)
        return
    passed = [a for a in sys.argv[1:]]
    for step in args.steps:
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--child", step] + passed)
        if r.returncode in (124, 137):
            sys.exit(f"refine_bench: step {step} did not finish in {LIMITS[step]} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"refine_bench: step {step} ended with status {r.returncode}; nothing further is started")


if __name__ == "__main__":
    main()
