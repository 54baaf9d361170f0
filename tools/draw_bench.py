#!/usr/bin/env python3
"""BGR frames and tracked skeletons in, painted frames and the encoder's NV12 surface out: kasf_draw_poses alone on the device, its bandwidth yardstick, and
the host path it replaces.

    python tools/draw_bench.py [--reps 7] [--kernel-iters 50] [--seed 0] [--step-timeout 180] [--out FILE.json]

1080 x 1920 frames of seeded noise on the device; P synthetic players: 17-joint figures 150..400 pixels tall around random centres.  Two steps, each a child
process of its own under its own time limit (--step-timeout seconds); the first step that fails, faults or runs out of time ends the run, nothing is started
after it.
  kernel     kasf_draw_poses alone at F = 1 and 16 frames, P = 0, 2 and 22 players, writing the BGR frame only, the surface only, or both (and, at P = 22, the
             frame in place): three warm-up launches, then CUDA events around --kernel-iters back-to-back launches, per launch, median and minimum of --reps,
             with GB/s of bytes READ + WRITTEN (3 read, 3 and / or 1.5 written per pixel).  In the same process, timed the same way, the yardstick:
             kasf_yuv420_to_bgr on the NV12 surfaces just written (1.5 read, 3 written per pixel).  The two ratios the binning and the empty tile answer for:
             P = 22 over P = 0, and P = 0 surface-only over the yardstick.
  host       the path the call replaces, for one frame and 22 players: the device-to-host copy of the frame and the keypoints, the numpy restatements of
             tests/test_draw_cpu.py (each primitive over its own box) and the upload of the NV12 surface, host clock, median of --reps; labelled "frame
             download + numpy restatement + surface upload".  It is NOT cv2: there is no OpenCV here.  The results of both ways are compared
             (equal_to_device).  Also the device call as a caller sees it (host clock up to a synchronise).
Prints one JSON line; --out also writes it to a file (stamp it with tools/stamp.py --embed).
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

HF, WF = 1080, 1920
STEPS = ("kernel", "host")
# a standing figure in units of its height, H36M joint order: x to the right, y downwards from the hip
FIGURE = ((0.0, 0.0), (0.07, 0.0), (0.08, 0.24), (0.08, 0.47), (-0.07, 0.0), (-0.08, 0.24), (-0.08, 0.47), (0.0, -0.13), (0.0, -0.27), (0.0, -0.33), (0.0, -0.42),
          (-0.10, -0.26), (-0.14, -0.12), (-0.15, 0.02), (0.10, -0.26), (0.14, -0.12), (0.15, 0.02))


def _players(seed, F, P):
    """[F,P,17,3] fp32: P figures per frame, 150..400 pixels tall, limbs jittered, scores 0.5..1."""
    import numpy as np
    g = np.random.default_rng(seed)
    height = g.uniform(150, 400, size=(F, P, 1, 1))
    centre = np.stack((g.uniform(100, WF - 100, size=(F, P, 1)), g.uniform(250, HF - 250, size=(F, P, 1))), axis=-1)
    xy = centre + height * (np.asarray(FIGURE)[None, None] + g.normal(0.0, 0.02, size=(F, P, 17, 2)))
    return np.concatenate([xy, g.uniform(0.5, 1.0, size=(F, P, 17, 1))], axis=-1).astype(np.float32)


def _timed(fn):
    """(result, CUDA-event ms, host wall ms) of fn() up to a synchronise after it."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def _per_launch(launch, reps, iters):
    from kasportsformer_amd import _lib
    for _ in range(3):
        _lib.check(launch())
    ms = [_timed(lambda: [_lib.check(launch()) for _ in range(iters)])[1] / iters for _ in range(reps)]
    return statistics.median(ms), min(ms)


def step_kernel(args):
    import numpy as np
    import torch
    from kasportsformer_amd import _lib, draw
    from kasportsformer_amd._args import stream
    lib = _lib.load()
    NF = 16
    frames = torch.from_numpy(np.random.default_rng(args.seed).integers(0, 256, size=(NF, HF, WF, 3), dtype=np.uint8)).cuda()
    out = torch.empty_like(frames)
    y = torch.empty((NF, HF, WF), dtype=torch.uint8, device="cuda")
    uv = torch.empty((NF, HF // 2, WF), dtype=torch.uint8, device="cuda")
    seg = torch.tensor(draw.H36M_SEGMENTS, dtype=torch.int32, device="cuda")
    col = torch.from_numpy(draw.hue_wheel(16)).cuda()
    dot = (C.c_uint8 * 3)(255, 255, 255)
    res = {"device": torch.cuda.get_device_name(0)}
    us = {}
    for n in (1, 16):
        for P in (0, 2, 22):
            kp = torch.from_numpy(_players(args.seed + P, NF, max(P, 1))).cuda()
            for what in ("bgr", "surface", "both") + (("in place",) if P == 22 else ()):
                o = {"bgr": out, "both": out, "in place": frames}.get(what)
                s = what in ("surface", "both")
                launch = (lambda o=o, s=s, P=P, kp=kp: lib.kasf_draw_poses(
                    frames.data_ptr(), n, HF, WF, 3 * WF, 3 * HF * WF, kp.data_ptr() if P else None, P, 17, 3, *kp.stride(), None, 0, 0, seg.data_ptr(),
                    col.data_ptr(), 16, dot, 2, 2, 0.25, None, 0, None if o is None else o.data_ptr(), 3 * WF, 3 * HF * WF, y.data_ptr() if s else None,
                    uv.data_ptr() if s else None, WF, WF, HF * WF, HF * WF // 2, _lib.YUV_BT601, 0, 0, stream()))
                med, best = _per_launch(launch, args.reps, args.kernel_iters)
                per_px = 3.0 + (3.0 if o is not None and what != "in place" else 0.0) + (1.5 if s else 0.0)
                nbytes = n * HF * WF * per_px
                us[(n, P, what)] = med * 1e3
                res[f"P={P} {what} @ F={n}"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "read_plus_written_MB": round(nbytes / 1e6, 2),
                                                "read_plus_written_GB_per_s": round(nbytes / med / 1e6, 1),
                                                **({"note": "in place only painted blocks are stored; the GB/s counts the read alone"} if what == "in place" else {})}
        # the yardstick, on the surfaces just written
        med, best = _per_launch(lambda: lib.kasf_yuv420_to_bgr(y.data_ptr(), uv.data_ptr(), None, _lib.YUV_NV12, n, HF, WF, WF, WF, HF * WF, HF * WF // 2, out.data_ptr(),
                                                               3 * WF, 3 * HF * WF, _lib.YUV_BT601, 0, 0, stream()), args.reps, args.kernel_iters)
        nbytes = n * HF * WF * 4.5
        us[(n, "yardstick")] = med * 1e3
        res[f"yardstick yuv420_to_bgr nv12 @ F={n}"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "read_plus_written_MB": round(nbytes / 1e6, 2),
                                                        "read_plus_written_GB_per_s": round(nbytes / med / 1e6, 1)}
        res[f"ratios @ F={n}"] = {"P=22 over P=0, both": round(us[(n, 22, "both")] / us[(n, 0, "both")], 3),
                                  "P=22 over P=0, surface": round(us[(n, 22, "surface")] / us[(n, 0, "surface")], 3),
                                  "P=0 surface over yardstick": round(us[(n, 0, "surface")] / us[(n, "yardstick")], 3)}
    return res


def step_host(args):
    import torch
    import kasportsformer_amd as K
    import numpy as np
    from tests.test_draw_cpu import bgr_to_nv12_np, draw_poses_np
    P = 22
    frame = torch.from_numpy(np.random.default_rng(args.seed).integers(0, 256, size=(HF, WF, 3), dtype=np.uint8)).cuda()
    kp = torch.from_numpy(_players(args.seed + P, 1, P)[0]).cuda()
    want = K.draw_poses(frame, kp, min_score=0.25, out=False, surface=True)
    colors = K.draw.hue_wheel(16)
    down_ms, np_ms, up_ms, total_ms = [], [], [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host, hkp = frame.cpu().numpy(), kp.cpu().numpy()
        t1 = time.perf_counter()
        painted = draw_poses_np(host[None], hkp[None], None, colors=colors, min_score=0.25, boxed=True)
        y, uv = bgr_to_nv12_np(painted[0])
        t2 = time.perf_counter()
        uy, uuv = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        down_ms.append((t1 - t0) * 1e3)
        np_ms.append((t2 - t1) * 1e3)
        up_ms.append((t3 - t2) * 1e3)
        total_ms.append((t3 - t0) * 1e3)
    wall = [_timed(lambda: K.draw_poses(frame, kp, min_score=0.25, out=False, surface=True))[2] for _ in range(args.reps)]
    return {"label": "frame download + numpy restatement + surface upload (NOT cv2: no OpenCV build at hand)", "frames": 1, "players": P,
            "download_ms": round(statistics.median(down_ms), 3), "numpy_ms": round(statistics.median(np_ms), 3), "upload_ms": round(statistics.median(up_ms), 3),
            "total_ms": round(statistics.median(total_ms), 3), "equal_to_device": bool(torch.equal(uy, want.y) and torch.equal(uuv, want.uv)),
            "device_call_wall_ms": round(statistics.median(wall), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"kernel": step_kernel, "host": step_host}[args.step](args)))
        return 0
    res = {"what": "frames and skeletons in, painted frames and NV12 surfaces out (measured; CUDA events for the device, host clock for the host path, median of %d)"
                   % args.reps, "frame": [HF, WF]}
    code = 0
    for step in STEPS:                                       # the parent never opens the GPU: each step is a fresh process under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--kernel-iters", str(args.kernel_iters), "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            res[step] = {"failed": f"no result within {args.step_timeout} s"}
            code = 1
            break
        if r.returncode != 0:
            res[step] = {"failed": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            code = 1
            break
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return code


if __name__ == "__main__":
    sys.exit(main())
