#!/usr/bin/env python3
"""Decoder surfaces in, BGR frames out: kasf_yuv420_to_bgr alone on the device, the host path it replaces, and two yardstick kernels.

    python tools/yuv_bench.py [--reps 7] [--kernel-iters 50] [--seed 0] [--step-timeout 120] [--out FILE.json]

1080 x 1920 surfaces of seeded noise on the device.  NV12 as a hardware decoder leaves it: pitch 2048, the UV plane at the aligned row 1088; I420 as packed
planes.  Three steps, each a child process of its own under its own time limit (--step-timeout seconds); the first step that fails, faults or runs out of
time ends the run, nothing is started after it.
  kernel     kasf_yuv420_to_bgr alone at F = 1 and 16 frames, NV12 and I420: three warm-up launches, then CUDA events around --kernel-iters back-to-back
             launches, per launch, median and minimum of --reps, with GB/s of INPUT + OUTPUT (F x 1080 x 1920 x 4.5 bytes: 1.5 read, 3 written per pixel).
             In the same process, timed the same way, the yardsticks: kasf_letterbox_frames at F = 16 (1080p -> 416, fp32) and kasf_crop_persons at 22
             persons (288 x 384 crops, fp32), the library's two frame-reading kernels, with GB/s of output.
  host       the path the call replaces, for one NV12 surface: the device-to-host copy of the surface, the numpy restatement of tests/test_yuv_cpu.py and the
             upload of the BGR frame (6.2 MB), host clock, median of --reps; labelled "surface download + numpy restatement + upload".  It is NOT cv2 /
             FFmpeg: there is no OpenCV here.  The results of both ways are compared (equal_to_device).  Also the device call as a caller sees it (host clock
             up to a synchronise).
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

HF, WF, PITCH, CHROMA_ROW, DIM = 1080, 1920, 2048, 1088, 416
ROWS = CHROMA_ROW + HF // 2
STEPS = ("kernel", "host")


def _surfaces(seed, n):
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, size=(n, ROWS, PITCH), dtype=np.uint8)


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
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import stream
    from tests.test_crop_cpu import MEAN, STD
    lib = _lib.load()
    nv12 = torch.from_numpy(_surfaces(args.seed, 16)).cuda()                                   # [16, ROWS, PITCH]
    y = nv12[:, :HF, :WF].contiguous()                                                         # I420: packed planes of the same samples
    uv = nv12[:, CHROMA_ROW:CHROMA_ROW + HF // 2, :WF].unflatten(-1, (WF // 2, 2))
    u, v = uv[..., 0].contiguous(), uv[..., 1].contiguous()
    frames = torch.empty((16, HF, WF, 3), dtype=torch.uint8, device="cuda")
    res = {"device": torch.cuda.get_device_name(0)}
    surface = ROWS * PITCH
    for n in (1, 16):
        calls = {
            "nv12": lambda: lib.kasf_yuv420_to_bgr(nv12.data_ptr(), nv12.data_ptr() + CHROMA_ROW * PITCH, None, _lib.YUV_NV12, n, HF, WF, PITCH, PITCH, surface,
                                                   surface, frames.data_ptr(), 3 * WF, 3 * HF * WF, _lib.YUV_BT601, 0, 0, stream()),
            "i420": lambda: lib.kasf_yuv420_to_bgr(y.data_ptr(), u.data_ptr(), v.data_ptr(), _lib.YUV_I420, n, HF, WF, WF, WF // 2, HF * WF, HF * WF // 4,
                                                   frames.data_ptr(), 3 * WF, 3 * HF * WF, _lib.YUV_BT601, 0, 0, stream()),
        }
        for name, launch in calls.items():
            med, best = _per_launch(launch, args.reps, args.kernel_iters)
            nbytes = n * HF * WF * 9 // 2
            res[f"{name} @ F={n}"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "input_plus_output_MB": round(nbytes / 1e6, 2),
                                      "input_plus_output_GB_per_s": round(nbytes / med / 1e6, 1)}
    # the yardsticks, on the frames just written
    out = torch.empty((16, 3, DIM, DIM), dtype=torch.float32, device="cuda")
    med, best = _per_launch(lambda: lib.kasf_letterbox_frames(frames.data_ptr(), 16, HF, WF, 3 * WF, HF * WF * 3, out.data_ptr(), _lib.DTYPE_F32, DIM, DIM, 128, 1,
                                                              stream()), args.reps, args.kernel_iters)
    nbytes = out.numel() * 4
    res["yardstick letterbox_frames fp32 @ F=16"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "output_MB": round(nbytes / 1e6, 2),
                                                     "output_GB_per_s": round(nbytes / med / 1e6, 1)}
    g = np.random.default_rng(args.seed)
    P, out_w, out_h = 22, 288, 384
    h = g.uniform(150, 700, P)
    w = h * g.uniform(0.3, 0.5, P)
    cx, cy = g.uniform(0, WF, P), g.uniform(0, HF, P)
    boxes = torch.from_numpy(np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), axis=-1).astype(np.float32)).cuda()
    cs = torch.empty((P, 4), device="cuda")
    crops = torch.empty((P, 3, out_h, out_w), dtype=torch.float32, device="cuda")
    ms_arr = (C.c_float * 6)(*MEAN, *STD)
    med, best = _per_launch(lambda: lib.kasf_crop_persons(frames.data_ptr(), 1, HF, WF, 3 * WF, 0, None, boxes.data_ptr(), _lib.GEOM_BOX, HF / WF, P,
                                                          crops.data_ptr(), _lib.DTYPE_F32, out_w, out_h, ms_arr, 1, cs.data_ptr(), stream()), args.reps,
                            args.kernel_iters)
    nbytes = crops.numel() * 4
    res[f"yardstick crop_persons fp32 @ n={P}"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "output_MB": round(nbytes / 1e6, 2),
                                                   "output_GB_per_s": round(nbytes / med / 1e6, 1)}
    return res


def step_host(args):
    import torch
    import kasportsformer_amd as K
    from tests.test_yuv_cpu import nv12_to_bgr_np
    surface = torch.from_numpy(_surfaces(args.seed, 1)[0]).cuda()
    want = K.nv12_to_bgr(surface, HF, WF, chroma_row=CHROMA_ROW)
    down_ms, np_ms, up_ms, total_ms = [], [], [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = surface.cpu().numpy()
        t1 = time.perf_counter()
        got = nv12_to_bgr_np(host, HF, WF, chroma_row=CHROMA_ROW)
        t2 = time.perf_counter()
        up = torch.from_numpy(got).cuda()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        down_ms.append((t1 - t0) * 1e3)
        np_ms.append((t2 - t1) * 1e3)
        up_ms.append((t3 - t2) * 1e3)
        total_ms.append((t3 - t0) * 1e3)
    wall = [_timed(lambda: K.nv12_to_bgr(surface, HF, WF, chroma_row=CHROMA_ROW))[2] for _ in range(args.reps)]
    return {"label": "surface download + numpy restatement + upload (NOT cv2 / FFmpeg: no OpenCV build at hand)", "frames": 1,
            "download_ms": round(statistics.median(down_ms), 3), "numpy_ms": round(statistics.median(np_ms), 3), "upload_ms": round(statistics.median(up_ms), 3),
            "total_ms": round(statistics.median(total_ms), 3), "equal_to_device": bool(torch.equal(up, want)),
            "device_call_wall_ms": round(statistics.median(wall), 4)}


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
        print(json.dumps({"kernel": step_kernel, "host": step_host}[args.step](args)))
        return 0
    res = {"what": "decoder surfaces in, BGR frames out (measured; CUDA events for the device, host clock for the host path, median of %d)" % args.reps,
           "surface": {"frame": [HF, WF], "nv12_pitch": PITCH, "nv12_chroma_row": CHROMA_ROW}}
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
