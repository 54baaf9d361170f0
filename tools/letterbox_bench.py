#!/usr/bin/env python3
"""Video frames in, detector inputs out: kasf_letterbox_frames alone on the device, the host path it replaces, and a yardstick kernel.

    python tools/letterbox_bench.py [--reps 7] [--kernel-iters 50] [--seed 0] [--step-timeout 120] [--out FILE.json]

1080 x 1920 BGR frames (seeded: smooth gradients plus noise) on the device, letterboxed to 416 x 416 (the demo's inp_dim).  Three steps, each a child process
of its own under its own time limit (--step-timeout seconds); the first step that fails, faults or runs out of time ends the run, nothing is started after it.
  kernel     kasf_letterbox_frames alone at F = 1 and 16 frames, fp32 and fp16 output: three warm-up launches, then CUDA events around --kernel-iters
             back-to-back launches, per launch, median and minimum of --reps, with GB/s of OUTPUT (F x 3 x 416 x 416 x element size; the frame bytes read
             are at most the 6.2 MB frame each, L2-resident).
  host       the path the call replaces, for one frame.  There is no OpenCV here, so this is NOT cv2.resize: it is the numpy restatement of
             tests/test_letterbox_cpu.py plus the host-to-device upload of its fp32 result (2 MB), host clock, median of --reps; labelled "numpy restatement +
             upload".  The results of both ways are compared.  Also the device call as a caller sees it (host clock up to a synchronise).
  yardstick  kasf_crop_persons at 22 persons (288 x 384 crops of the same frame, fp32 and fp16), timed the same way: the library's other frame-reading kernel,
             GB/s of output.
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

HF, WF, DIM = 1080, 1920, 416
STEPS = ("kernel", "host", "yardstick")


def _frames(seed, n):
    import numpy as np
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HF, 0:WF].astype(np.float32)
    planes = [128 + 60 * np.sin(0.011 * xx + c) * np.cos(0.007 * yy) + 40 * np.sin(0.004 * (xx + yy) + 2 * c) for c in range(3)]
    base = np.stack(planes, axis=-1)
    return np.stack([np.clip(np.rint(base + g.integers(-20, 21, size=(HF, WF, 3))), 0, 255).astype(np.uint8) for _ in range(n)])


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
    import torch
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import stream
    lib = _lib.load()
    frames = torch.from_numpy(_frames(args.seed, 16)).cuda()
    res = {"device": torch.cuda.get_device_name(0)}
    for n in (1, 16):
        for name, dt, code in (("fp32", torch.float32, _lib.DTYPE_F32), ("fp16", torch.float16, _lib.DTYPE_F16)):
            out = torch.empty((n, 3, DIM, DIM), dtype=dt, device="cuda")
            med, best = _per_launch(lambda: lib.kasf_letterbox_frames(frames.data_ptr(), n, HF, WF, 3 * WF, HF * WF * 3, out.data_ptr(), code, DIM, DIM, 128, 1,
                                                                      stream()), args.reps, args.kernel_iters)
            nbytes = out.numel() * out.element_size()
            res[f"{name} @ F={n}"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "output_MB": round(nbytes / 1e6, 2),
                                      "output_GB_per_s": round(nbytes / med / 1e6, 1)}
    return res


def step_host(args):
    import torch
    import kasportsformer_amd as K
    from tests.test_letterbox_cpu import letterbox_np
    frame_h = _frames(args.seed, 1)[0]
    frame = torch.from_numpy(frame_h).cuda()
    want = K.letterbox_frames(frame, DIM).inputs
    np_ms, up_ms, total_ms = [], [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = letterbox_np(frame_h, DIM)
        t1 = time.perf_counter()
        up = torch.from_numpy(got).cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        np_ms.append((t1 - t0) * 1e3)
        up_ms.append((t2 - t1) * 1e3)
        total_ms.append((t2 - t0) * 1e3)
    wall = [_timed(lambda: K.letterbox_frames(frame, DIM))[2] for _ in range(args.reps)]
    return {"label": "numpy restatement + upload (NOT cv2.resize: no OpenCV build at hand)", "frames": 1, "numpy_ms": round(statistics.median(np_ms), 3),
            "upload_ms": round(statistics.median(up_ms), 3), "total_ms": round(statistics.median(total_ms), 3), "equal_to_device": bool(torch.equal(up, want)),
            "device_call_wall_ms": round(statistics.median(wall), 4)}


def step_yardstick(args):
    import numpy as np
    import torch
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import stream
    from tests.test_crop_cpu import MEAN, STD
    lib = _lib.load()
    g = np.random.default_rng(args.seed)
    frame = torch.from_numpy(_frames(args.seed, 1)[0]).cuda()
    n, out_w, out_h = 22, 288, 384
    h = g.uniform(150, 700, n)
    w = h * g.uniform(0.3, 0.5, n)
    cx, cy = g.uniform(0, WF, n), g.uniform(0, HF, n)
    boxes = torch.from_numpy(np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), axis=-1).astype(np.float32)).cuda()
    cs = torch.empty((n, 4), device="cuda")
    ms_arr = (C.c_float * 6)(*MEAN, *STD)
    res = {}
    for name, dt, code in (("fp32", torch.float32, _lib.DTYPE_F32), ("fp16", torch.float16, _lib.DTYPE_F16)):
        out = torch.empty((n, 3, out_h, out_w), dtype=dt, device="cuda")
        med, best = _per_launch(lambda: lib.kasf_crop_persons(frame.data_ptr(), 1, HF, WF, 3 * WF, 0, None, boxes.data_ptr(), _lib.GEOM_BOX, HF / WF, n,
                                                              out.data_ptr(), code, out_w, out_h, ms_arr, 1, cs.data_ptr(), stream()), args.reps, args.kernel_iters)
        nbytes = out.numel() * out.element_size()
        res[f"crop_persons {name} @ n={n}"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "output_MB": round(nbytes / 1e6, 2),
                                               "output_GB_per_s": round(nbytes / med / 1e6, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"kernel": step_kernel, "host": step_host, "yardstick": step_yardstick}[args.step](args)))
        return 0
    res = {"what": "video frames in, detector inputs out (measured; CUDA events for the device, host clock for the host path, median of %d)" % args.reps,
           "frame": [HF, WF, 3], "input": [DIM, DIM]}
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
