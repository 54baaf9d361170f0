#!/usr/bin/env python3
"""The camera-space placement on the device (kasportsformer_amd.place_poses, kasf_pose_place) next to a pure streaming kernel over the same poses and the host
path it replaces.

    python tools/place_bench.py [--steps launches host] [--iters 20] [--reps 5] [--seed 0]

Every step runs in a child process of its own under its own `timeout -k 10`, one after the other; a step that fails or runs out of time ends the run.
  launches  kasf_pose_place alone over synthetic players (tests/place_ref.py's scenes with a pixel of noise) at one 18,000-frame track and at 22 x 1,800
            frames, with iterations 0 and 4, without and with a bone table.  CUDA events around --iters back-to-back calls of the C entry, per call, the median
            of --reps; GB/s of the 633 bytes per frame it reads and writes (poses, keypoints, out, root, residual, scale, state).  In the same run, over the same
            poses, kasf_pose_world (408 bytes per frame) as the bandwidth yardstick, and the ratio of the two times.
  host      the path it replaces for the same inputs: download of poses and keypoints, the numpy restatement of the rule (tests/place_ref.py), upload of the
            results; host clock up to a synchronise; its results are compared with the device's on their bits.
Prints one JSON line per measurement, the last with the source stamp.  None of the numbers is a pass / fail bar.
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
SIZES = {"one track of 18,000": 18000, "22 x 1,800": 22 * 1800}
BYTES_PLACE, BYTES_WORLD = 3 * 204 + 12 + 4 + 4 + 1, 2 * 204


def _events(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _players(np, n, seed):
    from tests.place_ref import BONES_170, scene
    g = np.random.default_rng(seed)
    P, _, K, camera = scene(g, n)
    K[..., :2] += g.normal(0.0, 1.0, (n, 17, 2)).astype(np.float32)
    return P, K, camera, BONES_170.copy()


def step_launches(args):
    import ctypes as C
    import numpy as np
    import torch
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import stream
    from kasportsformer_amd.place import place_params
    from kasportsformer_amd.pose import DEMO_CAMERA_ROTATION
    lib = _lib.load()
    for size, N in SIZES.items():
        P, K, camera, table = _players(np, N, args.seed)
        Pd, Kd, cd, td = (torch.from_numpy(a).cuda() for a in (P, K, camera, table))
        out, root = torch.empty_like(Pd), torch.empty((N, 3), device="cuda")
        residual, scale, state = torch.empty(N, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")

        def timed(fn):
            fn()
            return statistics.median(_events(torch, fn, args.iters) for _ in range(args.reps))
        q4, t3 = np.asarray(DEMO_CAMERA_ROTATION, np.float32), np.zeros(3, np.float32)
        world_ms = timed(lambda: _lib.check(lib.kasf_pose_world(Pd.data_ptr(), N, q4.ctypes.data, t3.ctypes.data, 0, 0, out.data_ptr(), stream())))
        print(json.dumps({"what": "kasf_pose_world (yardstick: a streaming kernel over the same poses)", "size": size, "frames": N, "event_ms": round(world_ms, 5),
                          "GBps": round(N * BYTES_WORLD / world_ms / 1e6, 2), "device": torch.cuda.get_device_name(0)}), flush=True)
        for iterations in (0, 4):
            for with_table in (False, True):
                q = place_params(iterations=iterations)
                ms = timed(lambda: _lib.check(lib.kasf_pose_place(Pd.data_ptr(), Kd.data_ptr(), N, cd.data_ptr(), 0, td.data_ptr() if with_table else None, 0,
                                                                  C.byref(q), out.data_ptr(), root.data_ptr(), residual.data_ptr(), scale.data_ptr(),
                                                                  state.data_ptr(), stream())))
                print(json.dumps({"what": "kasf_pose_place", "size": size, "frames": N, "iterations": iterations, "table": with_table, "event_ms": round(ms, 5),
                                  "GBps": round(N * BYTES_PLACE / ms / 1e6, 2), "ratio_to_pose_world": round(ms / world_ms, 2),
                                  "byte_ratio": round(BYTES_PLACE / BYTES_WORLD, 2), "placed": int((state == 0).sum())}), flush=True)


def step_host(args):
    import numpy as np
    import torch
    import kasportsformer_amd as K_
    from tests.place_ref import place_np
    for size, N in SIZES.items():
        P, K, camera, table = _players(np, N, args.seed)
        Pd, Kd = torch.from_numpy(P).cuda(), torch.from_numpy(K).cuda()
        K_.place_poses(Pd, Kd, camera, metric_lengths=table)

        def host():
            r = place_np(Pd.cpu().numpy(), Kd.cpu().numpy(), camera, table)
            return K_.PlaceResult(*(torch.from_numpy(r[k]).cuda() for k in ("poses", "root", "residual", "scale", "state")))
        wall = {}
        for name, fn in (("device", lambda: K_.place_poses(Pd, Kd, camera, metric_lengths=table)), ("host", host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            wall[name] = ((time.perf_counter() - t0) * 1e3, [t.cpu().numpy().view(np.uint8) for t in got])
        print(json.dumps({"what": "place_poses vs download + numpy restatement + upload, host clock", "size": size, "frames": N,
                          "device_wall_ms": round(wall["device"][0], 4), "host_path_wall_ms": round(wall["host"][0], 2),
                          "bits_equal": all(bool(np.array_equal(a, b)) for a, b in zip(wall["device"][1], wall["host"][1]))}), flush=True)
    from tools.stamp import stamp
    print(json.dumps({"stamp": stamp()}), flush=True)


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
            sys.exit("place_bench: needs a GPU; there is no CPU path to time")
        STEPS[args.child](args)
        return
    passed = [a for a in sys.argv[1:]]
    for step in args.steps:
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--child", step] + passed)
        if r.returncode in (124, 137):
            sys.exit(f"place_bench: step {step} did not finish in {LIMITS[step]} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"place_bench: step {step} ended with status {r.returncode}; nothing further is started")


if __name__ == "__main__":
    main()
