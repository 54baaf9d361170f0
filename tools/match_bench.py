#!/usr/bin/env python3
"""Matching players across cameras on the device (kasportsformer_amd.match_players; kasf_match_pair_costs, kasf_match_groups) next to the triangulation over
the same keypoint bytes and the host path it replaces.

    python tools/match_bench.py [--steps launches host] [--iters 5] [--reps 5] [--seed 0] [--frames 18000] [--cameras 7] [--rows 22] [--host-frames 512]

Every step runs in a child process of its own under its own `timeout -k 10`, one after the other; a step that fails or runs out of time ends the run.
  launches  kasf_match_pair_costs alone over --rows rows in each of --cameras cameras on a ring (tests/match_ref.scene: a pixel of noise, a lens, every camera
            its own row order; a base of 1,000 frames repeated up to --frames) at --frames frames of 17 joints and at one live tick, N = 1; kasf_match_groups
            alone over the costs of the long call; kasf_keypoints_triangulate (4 iterations) over the same keypoint bytes as the in-run yardstick.  CUDA events
            around --iters back-to-back calls of the C entry, per call, the median of --reps.  For the pair costs: the compared samples per second, the fp64
            operations per second at 71 per compared sample (a divide or a square root counted as one; the undistortion is not counted), and the keypoint
            bytes (12 per sample of every row) per second.
  host      the path it replaces: download + the numpy restatement (tests/match_ref.pair_costs_np and groups_np, the bit-exact one, whose sums walk the samples
            one by one) + upload, host clock up to a synchronise, over the first --host-frames frames only -- at 18,000 frames it runs for many minutes -- with
            the time at --frames extrapolated in proportion and labelled so; its results are compared with the device's on their bits.
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
LIMITS = {"launches": 240, "host": 420}                            # seconds per child
OPS_PER_SAMPLE = 71


def _events(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _tracks(np, frames, cameras, rows, seed):
    """K [cameras, rows, frames, 17, 3], cams [cameras, 21]: rows - 1 players and an empty row, a base of at most 1,000 frames repeated."""
    from tests.match_ref import scene
    base = min(frames, 1000)
    K, cams, _, _ = scene(frames=base, cameras=cameras, players=rows - 1, joints=17, pad=1, seed=seed)
    K = np.concatenate([K] * ((frames + base - 1) // base), 2)[:, :, :frames]
    return np.ascontiguousarray(K), cams


def step_launches(args):
    import ctypes as C
    import numpy as np
    import torch
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import stream
    from kasportsformer_amd.match import match_params
    from kasportsformer_amd.triangulate import triangulate_params
    lib = _lib.load()
    V, P, N = args.cameras, args.rows, args.frames
    K, cams = _tracks(np, N, V, P, args.seed)
    Kd, cd = torch.from_numpy(K).cuda(), torch.from_numpy(cams).cuda()
    cost, samples = torch.empty((V, V, P, P), device="cuda"), torch.empty((V, V, P, P), dtype=torch.int32, device="cuda")
    q = match_params(17)

    def timed(fn):
        fn()
        return statistics.median(_events(torch, fn, args.iters) for _ in range(args.reps))
    for n in (N, 1):
        kn = Kd[:, :, :n].contiguous()
        nbytes = int(lib.kasf_match_workspace_bytes(V, P, n))
        work = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
        ms = timed(lambda: _lib.check(lib.kasf_match_pair_costs(kn.data_ptr(), V, P, n, 17, cd.data_ptr(), C.byref(q), cost.data_ptr(), samples.data_ptr(),
                                                                work.data_ptr(), nbytes, stream())))
        compared = int(samples.sum().item()) // 2
        possible = V * (V - 1) // 2 * P * P * n * 17
        print(json.dumps({"what": "kasf_match_pair_costs", "cameras": V, "rows": P, "frames": n, "joints": 17, "event_ms": round(ms, 5),
                          "ray_pairs": possible, "compared_samples": compared, "compared_Gsamples_per_s": round(compared / ms / 1e6, 3),
                          "fp64_Gops_per_s": round(compared * OPS_PER_SAMPLE / ms / 1e6, 1), "keypoint_bytes": kn.numel() * 4,
                          "keypoint_GBps": round(kn.numel() * 4 / ms / 1e6, 3), "workspace_bytes": nbytes, "device": torch.cuda.get_device_name(0)}), flush=True)
        if n == N:
            G = min(64, 2 * P)
            outs = [torch.empty(s, dtype=t, device="cuda") for s, t in (((V, P), torch.int32), ((G, V), torch.int32), ((G,), torch.int32), ((G,), torch.float32),
                                                                       ((), torch.int32), ((), torch.int32))]
            gms = timed(lambda: _lib.check(lib.kasf_match_groups(cost.data_ptr(), samples.data_ptr(), V, P, 15.0, G, *[o.data_ptr() for o in outs], stream())))
            print(json.dumps({"what": "kasf_match_groups", "cameras": V, "rows": P, "max_groups": G, "event_ms": round(gms, 5), "groups": int(outs[4]),
                              "dropped": int(outs[5])}), flush=True)
            M = P * n * 17                                              # the same bytes as one point set of `cameras` views
            points, residual = torch.empty((M, 3), device="cuda"), torch.empty(M, device="cuda")
            used, state = torch.empty(M, dtype=torch.uint8, device="cuda"), torch.empty(M, dtype=torch.uint8, device="cuda")
            t = triangulate_params()
            tms = timed(lambda: _lib.check(lib.kasf_keypoints_triangulate(kn.data_ptr(), V, M, 17, cd.data_ptr(), 0, C.byref(t), points.data_ptr(),
                                                                          residual.data_ptr(), used.data_ptr(), state.data_ptr(), None, stream())))
            print(json.dumps({"what": "kasf_keypoints_triangulate (yardstick: the same keypoint bytes, 4 iterations)", "points": M, "views": V,
                              "event_ms": round(tms, 5), "keypoint_GBps": round(kn.numel() * 4 / tms / 1e6, 2), "pair_costs_over_triangulate": round(ms / tms, 2)}),
                  flush=True)


def step_host(args):
    import numpy as np
    import torch
    import kasportsformer_amd as K_
    from tests.match_ref import groups_np, pair_costs_np
    V, P, N = args.cameras, args.rows, min(args.host_frames, args.frames)
    K, cams = _tracks(np, N, V, P, args.seed)
    Kd = torch.from_numpy(K).cuda()
    K_.match_players(Kd, cams)
    names = ("group", "members", "views", "group_cost", "count", "dropped", "cost", "samples")

    def host():
        cost, samples = pair_costs_np(Kd.cpu().numpy(), cams)
        g = groups_np(cost, samples)
        return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in [g[k] for k in names[:6]] + [cost, samples]]
    wall = {}
    for name, fn in (("device", lambda: list(K_.match_players(Kd, cams))), ("host", host)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        wall[name] = ((time.perf_counter() - t0) * 1e3, [t.cpu().numpy().reshape(-1).view(np.uint8) for t in got])
    print(json.dumps({"what": "match_players vs download + the numpy restatement + upload; host clock", "cameras": V, "rows": P, "frames": N,
                      "device_wall_ms": round(wall["device"][0], 4), "host_path_wall_ms": round(wall["host"][0], 1),
                      "host_path_wall_ms_extrapolated_in_proportion_to_frames": {"frames": args.frames, "ms": round(wall["host"][0] * args.frames / N, 0)},
                      "bits_equal": all(bool(np.array_equal(a, b)) for a, b in zip(wall["device"][1], wall["host"][1]))}), flush=True)
    from tools.stamp import stamp
    print(json.dumps({"stamp": stamp()}), flush=True)


STEPS = {"launches": step_launches, "host": step_host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", choices=list(STEPS), default=list(STEPS))
    ap.add_argument("--child", choices=list(STEPS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=18000)
    ap.add_argument("--cameras", type=int, default=7)
    ap.add_argument("--rows", type=int, default=22)
    ap.add_argument("--host-frames", type=int, default=512)
    args = ap.parse_args()
    if args.child is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("match_bench: needs a GPU; there is no CPU path to time")
        STEPS[args.child](args)
        return
    passed = [a for a in sys.argv[1:]]
    for step in args.steps:
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--child", step] + passed)
        if r.returncode in (124, 137):
            sys.exit(f"match_bench: step {step} did not finish in {LIMITS[step]} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"match_bench: step {step} ended with status {r.returncode}; nothing further is started")


if __name__ == "__main__":
    main()
