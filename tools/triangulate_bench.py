#!/usr/bin/env python3
"""The multi-camera triangulation on the device (kasportsformer_amd.triangulate_keypoints, kasf_keypoints_triangulate) next to the undistortion alone, the
camera-space placement over the same frames and the host path it replaces.

    python tools/triangulate_bench.py [--steps launches host] [--iters 20] [--reps 5] [--seed 0] [--frames 18000] [--views 7]

Every step runs in a child process of its own under its own `timeout -k 10`, one after the other; a step that fails or runs out of time ends the run.
  launches  kasf_keypoints_triangulate alone over one synthetic player in --views cameras on a ring (tests/triangulate_ref.py: a pixel of noise, a lens), one
            track of --frames frames of 17 joints, with iterations 0 and 4, with and without the per-view residuals.  CUDA events around --iters back-to-back
            calls of the C entry, per call, the median of --reps; GB/s of the 12 C + 18 (+ 4 C) bytes per point it reads and writes.  In the same run:
            kasf_keypoints_undistort alone over one camera's track (24 bytes per point), and kasf_pose_place over the same number of frames (633 bytes per
            frame, iterations 0 and 4) as the yardstick, with the ratio of the times.
  host      the path it replaces for the same inputs: download, the numpy restatement vectorised (tests/triangulate_ref.triangulate_np), upload; host clock up
            to a synchronise; its results are compared with the device's on their bits.
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
BYTES_PLACE = 3 * 204 + 12 + 4 + 4 + 1


def _events(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _track(np, frames, views, seed):
    """One player's keypoints [views, frames * 17, 3] in a static rig [views, 21] with a lens: a pixel of noise, scores in [0.5, 1]."""
    from tests.triangulate_ref import LENS, players, project, ring
    g = np.random.default_rng(seed)
    cams = ring(views, g, distortion=LENS)
    uv = project(players(g, frames), cams)
    K = np.concatenate([uv + g.normal(0.0, 1.0, uv.shape), g.uniform(0.5, 1.0, uv.shape[:-1] + (1,))], -1).astype(np.float32)
    return np.ascontiguousarray(K), cams


def step_launches(args):
    import ctypes as C
    import numpy as np
    import torch
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import stream
    from kasportsformer_amd.place import place_params
    from kasportsformer_amd.triangulate import triangulate_params
    from tests.place_ref import scene
    lib = _lib.load()
    N, V = args.frames, args.views
    M = N * 17
    K, cams = _track(np, N, V, args.seed)
    Kd, cd = torch.from_numpy(K).cuda(), torch.from_numpy(cams).cuda()
    points, residual = torch.empty((M, 3), device="cuda"), torch.empty(M, device="cuda")
    used, state = torch.empty(M, dtype=torch.uint8, device="cuda"), torch.empty(M, dtype=torch.uint8, device="cuda")
    per_view, und = torch.empty((V, M), device="cuda"), torch.empty((M, 3), device="cuda")

    def timed(fn):
        fn()
        return statistics.median(_events(torch, fn, args.iters) for _ in range(args.reps))
    P, _, Kp, camera = scene(np.random.default_rng(args.seed), N)
    Pd, Kpd, camd = (torch.from_numpy(a).cuda() for a in (P, Kp, camera))
    out, root = torch.empty_like(Pd), torch.empty((N, 3), device="cuda")
    res_p, scale, st_p = torch.empty(N, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
    place_ms = {}
    for iterations in (0, 4):
        q = place_params(iterations=iterations)
        place_ms[iterations] = timed(lambda: _lib.check(lib.kasf_pose_place(Pd.data_ptr(), Kpd.data_ptr(), N, camd.data_ptr(), 0, None, 0, C.byref(q), out.data_ptr(),
                                                                            root.data_ptr(), res_p.data_ptr(), scale.data_ptr(), st_p.data_ptr(), stream())))
        print(json.dumps({"what": "kasf_pose_place (yardstick: the same frames, one lane per frame)", "frames": N, "iterations": iterations,
                          "event_ms": round(place_ms[iterations], 5), "GBps": round(N * BYTES_PLACE / place_ms[iterations] / 1e6, 2),
                          "device": torch.cuda.get_device_name(0)}), flush=True)
    ms = timed(lambda: _lib.check(lib.kasf_keypoints_undistort(Kd.data_ptr(), M, 17, cd.data_ptr(), 0, 5, und.data_ptr(), stream())))
    print(json.dumps({"what": "kasf_keypoints_undistort", "frames": N, "points": M, "rounds": 5, "event_ms": round(ms, 5), "GBps": round(M * 24 / ms / 1e6, 2),
                      "ratio_to_pose_place_0": round(ms / place_ms[0], 2)}), flush=True)
    for iterations in (0, 4):
        for views_out in (False, True):
            q = triangulate_params(iterations=iterations)
            ms = timed(lambda: _lib.check(lib.kasf_keypoints_triangulate(Kd.data_ptr(), V, M, 17, cd.data_ptr(), 0, C.byref(q), points.data_ptr(), residual.data_ptr(),
                                                                         used.data_ptr(), state.data_ptr(), per_view.data_ptr() if views_out else None, stream())))
            nbytes = 12 * V + 18 + (4 * V if views_out else 0)
            print(json.dumps({"what": "kasf_keypoints_triangulate", "frames": N, "points": M, "views": V, "iterations": iterations, "view_residual": views_out,
                              "event_ms": round(ms, 5), "GBps": round(M * nbytes / ms / 1e6, 2), "bytes_per_point": nbytes,
                              "ratio_to_pose_place": round(ms / place_ms[iterations], 2), "triangulated": int((state == 0).sum())}), flush=True)


def step_host(args):
    import numpy as np
    import torch
    import kasportsformer_amd as K_
    from tests.triangulate_ref import triangulate_np
    N, V = args.frames, args.views
    K, cams = _track(np, N, V, args.seed)
    Kd = torch.from_numpy(K.reshape(V, N, 17, 3)).cuda()
    K_.triangulate_keypoints(Kd, cams, view_residual=True)
    names = ("points", "residual", "used", "state", "view_residual")

    def host():
        r = triangulate_np(Kd.cpu().numpy().reshape(V, -1, 3), cams, 17)
        return [torch.from_numpy(r[k]).cuda() for k in names]
    wall = {}
    for name, fn in (("device", lambda: list(K_.triangulate_keypoints(Kd, cams, view_residual=True))), ("host", host)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        wall[name] = ((time.perf_counter() - t0) * 1e3, [t.cpu().numpy().reshape(-1).view(np.uint8) for t in got])
    print(json.dumps({"what": "triangulate_keypoints vs download, the numpy restatement vectorised, upload; host clock", "frames": N, "views": V,
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
    ap.add_argument("--frames", type=int, default=18000)
    ap.add_argument("--views", type=int, default=7)
    args = ap.parse_args()
    if args.child is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("triangulate_bench: needs a GPU; there is no CPU path to time")
        STEPS[args.child](args)
        return
    passed = [a for a in sys.argv[1:]]
    for step in args.steps:
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--child", step] + passed)
        if r.returncode in (124, 137):
            sys.exit(f"triangulate_bench: step {step} did not finish in {LIMITS[step]} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"triangulate_bench: step {step} ended with status {r.returncode}; nothing further is started")


if __name__ == "__main__":
    main()
