#!/usr/bin/env python3
"""Person boxes in, pose-network inputs out: kasf_crop_persons alone on the device, the host path it replaces, and two yardstick kernels.

    python tools/crop_bench.py [--reps 7] [--kernel-iters 50] [--host-persons 22] [--seed 0] [--out FILE.json]

A 1920 x 1080 BGR frame (seeded: smooth gradients plus noise) on the device, crops of 288 x 384 (the reference's MODEL.IMAGE_SIZE), boxes of standing persons
spread over the frame, some over its edges.
  crop     kasf_crop_persons alone at 1, 22 and 256 persons, fp32 and fp16 output: three warm-up launches, then CUDA events around --kernel-iters
           back-to-back launches, per launch, median and minimum of --reps, with GB/s of OUTPUT (persons x 3 x 384 x 288 x element size; the frame bytes
           read are at most the 6.2 MB frame, L2-resident).
  host     the path the call replaces, for the same frame and boxes.  There is no OpenCV here, so this is NOT cv2.warpAffine: it is the numpy restatement of
           tests/test_crop_cpu.py (vectorised per person) plus the host-to-device upload of its fp32 result, host clock, median of --reps, at
           --host-persons persons; labelled "numpy restatement + upload".  The crops of both ways are compared.
  yardsticks  achieved bytes/s of two kernels of this library that also stream: kasf_heatmap_keypoints (fp32 maps of 17 x 96 x 72 at 1,024 persons: bytes
           read) and kasf_lift_windows (flip, 1,000,000 frames: 612 bytes per frame read + written), timed the same way.
Prints one JSON line; --out also writes it to a file (stamp it with tools/stamp.py --embed).
"""
import argparse
import ctypes as C
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
from kasportsformer_amd.lift import window_plan  # noqa: E402
from kasportsformer_amd._args import stream  # noqa: E402
from tests.test_crop_cpu import MEAN, STD, crop_persons_np  # noqa: E402

HF, WF, OUT_W, OUT_H = 1080, 1920, 288, 384


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


def _per_launch(launch, reps, iters):
    for _ in range(3):
        _lib.check(launch())
    ms = [_timed(lambda: [_lib.check(launch()) for _ in range(iters)])[1] / iters for _ in range(reps)]
    return statistics.median(ms), min(ms)


def _frame(seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:HF, 0:WF].astype(np.float32)
    planes = [128 + 60 * np.sin(0.011 * xx + c) * np.cos(0.007 * yy) + 40 * np.sin(0.004 * (xx + yy) + 2 * c) for c in range(3)]
    f = np.stack(planes, axis=-1) + g.integers(-20, 21, size=(HF, WF, 3))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _boxes(g, n):
    """Standing persons 150 - 700 px tall, 0.3 - 0.5 as wide, centers anywhere in the frame (so some boxes cross its edges)."""
    h = g.uniform(150, 700, n)
    w = h * g.uniform(0.3, 0.5, n)
    cx, cy = g.uniform(0, WF, n), g.uniform(0, HF, n)
    return np.stack((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), axis=-1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--host-persons", type=int, default=22)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = np.random.default_rng(args.seed)
    lib = _lib.load()
    frame_h = _frame(args.seed)
    frame = torch.from_numpy(frame_h).cuda()
    ms_arr = (C.c_float * 6)(*MEAN, *STD)
    res = {"what": "person boxes in, pose-network inputs out (measured; CUDA events for the device, host clock for the host path, median of %d)" % args.reps,
           "frame": [HF, WF, 3], "crop": [OUT_H, OUT_W], "device": torch.cuda.get_device_name(0)}

    crop = {}
    for n in (1, 22, 256):
        boxes = torch.from_numpy(_boxes(g, n)).cuda()
        cs = torch.empty((n, 4), device="cuda")
        for name, dt, code in (("fp32", torch.float32, _lib.DTYPE_F32), ("fp16", torch.float16, _lib.DTYPE_F16)):
            out = torch.empty((n, 3, OUT_H, OUT_W), dtype=dt, device="cuda")

            def launch():
                return lib.kasf_crop_persons(frame.data_ptr(), 1, HF, WF, 3 * WF, 0, None, boxes.data_ptr(), _lib.GEOM_BOX, HF / WF, n, out.data_ptr(), code,
                                             OUT_W, OUT_H, ms_arr, 1, cs.data_ptr(), stream())
            med, best = _per_launch(launch, args.reps, args.kernel_iters)
            nbytes = out.numel() * out.element_size()
            crop[f"{name} @ n={n}"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "output_MB": round(nbytes / 1e6, 2),
                                       "output_GB_per_s": round(nbytes / med / 1e6, 1)}
            del out
    res["crop_kernel"] = crop

    # the host path: numpy restatement + upload of its fp32 result, against the device call as a caller sees it
    n = args.host_persons
    boxes_h = _boxes(g, n)
    want = K.crop_persons(frame, boxes_h).inputs
    np_ms, up_ms, total_ms = [], [], []
    for _ in range(max(1, args.reps // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = crop_persons_np(frame_h, boxes_h)[0]
        t1 = time.perf_counter()
        up = torch.from_numpy(got).cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        np_ms.append((t1 - t0) * 1e3)
        up_ms.append((t2 - t1) * 1e3)
        total_ms.append((t2 - t0) * 1e3)
    wall = [_timed(lambda: K.crop_persons(frame, boxes_h))[2] for _ in range(args.reps)]
    res["host_path"] = {"label": "numpy restatement + upload (NOT cv2.warpAffine: no OpenCV build at hand)", "persons": n,
                        "numpy_ms": round(statistics.median(np_ms), 3), "upload_ms": round(statistics.median(up_ms), 3),
                        "total_ms": round(statistics.median(total_ms), 3), "equal_to_device": bool(torch.equal(up, want)),
                        "device_call_wall_ms": round(statistics.median(wall), 4)}
    del want, up

    # yardsticks
    yard = {}
    H, W, nh = 96, 72, 1024
    hm = torch.rand((nh, 17, H, W), device="cuda")
    geom = torch.cat((torch.rand((nh, 2), device="cuda") * 1000, 1 + torch.rand((nh, 2), device="cuda")), dim=-1).contiguous()
    kp = torch.empty((nh, 17, 3), device="cuda")
    med, best = _per_launch(lambda: lib.kasf_heatmap_keypoints(hm.data_ptr(), _lib.DTYPE_F32, nh, H, W, geom.data_ptr(), _lib.GEOM_CENTER_SCALE, 1.0, 1,
                                                               _lib.LAYOUT_COCO, kp.data_ptr(), None, stream()), args.reps, args.kernel_iters)
    nbytes = hm.numel() * 4 + geom.numel() * 4 + kp.numel() * 4
    yard["heatmap_keypoints fp32 @ n=1024"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "GB_per_s": round(nbytes / med / 1e6, 1)}
    del hm
    T, frames = 27, 1000000
    src = torch.rand((frames, 17, 3), device="cuda")
    x = torch.empty((2 * len(window_plan(frames, T)[0]), T, 17, 3), device="cuda")
    r = window_plan(frames, T)[2]
    r_d = torch.from_numpy(r).cuda() if r is not None else None
    med, best = _per_launch(lambda: lib.kasf_lift_windows(src.data_ptr(), 1, frames, 1280.0, 720.0, T, T, r_d.data_ptr() if r_d is not None else None, 1,
                                                          x.data_ptr(), stream()), args.reps, args.kernel_iters)
    yard["lift_windows flip @ 1000000 frames"] = {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "GB_per_s": round(612 * frames / med / 1e6, 1)}
    res["yardsticks"] = yard
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
