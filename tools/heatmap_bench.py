#!/usr/bin/env python3
"""Pose-network heatmaps in, keypoints out: the decode on the device against the host path it replaces, and the live-stream tick that starts at heatmaps.

    python tools/heatmap_bench.py [--layers 26] [--dtype bf16] [--reps 7] [--kernel-iters 50] [--ticks 200] [--warmup 40] [--seed 0]

Heatmaps of HRNet-w48 at 384 x 288: 17 maps of 96 x 72 per person, seeded Gaussian blobs plus noise, on the device (where the pose network leaves them).
  decode   kasf_heatmap_keypoints alone (refine on, COCO out) at n = 22 and n = 1,024 persons, fp32 and fp16 maps: CUDA events around --kernel-iters
           back-to-back launches, per launch, median of --reps, with achieved GB/s (heatmap bytes read + geometry read + keypoints written).  The same
           with layout="h36m" (the second launch, kasf_coco_h36m) at n = 22.
  host     the path it replaces, for the same inputs: the device-to-host copy of the maps (demo/lib/hrnet/gen_kpts.py:158: output.clone().cpu().numpy())
           plus tests/test_heatmap_cpu.py's numpy restatement of get_final_preds (vectorised argmax, a Python loop over the 17 n refinements -- the
           reference loops in Python over all of it), host clock, median of --reps; the keypoints of both ways are compared.
  stream   22 slots, lag 0, the shipped model (26 layers, 8 heads, T = 27, bf16; random weights, which the time does not depend on), flip-TTA:
           StreamLifter.push_heatmaps of fp32 maps per tick against StreamLifter.push of ready H36M keypoints, alternating within the tick, CUDA events,
           median and 99th percentile of --ticks ticks after --warmup.
Prints one JSON line.
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
from tests.test_heatmap_cpu import heatmap_decode_np  # noqa: E402

T, W_PX, H_PX, H, W = 27, 1280, 720, 96, 72


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


def _stats(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "p99": round(v[min(len(v) - 1, int(0.99 * len(v)))], 4)}


def _maps(seed, n):
    """[n,17,H,W] fp32 on the device: one Gaussian blob per map (sigma 2, random center and amplitude) plus uniform noise of 2 % of full scale."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cy = torch.rand((n, 17, 1, 1), device="cuda", generator=g) * H
    cx = torch.rand((n, 17, 1, 1), device="cuda", generator=g) * W
    amp = 0.3 + 0.7 * torch.rand((n, 17, 1, 1), device="cuda", generator=g)
    yy = torch.arange(H, device="cuda").view(1, 1, H, 1)
    xx = torch.arange(W, device="cuda").view(1, 1, 1, W)
    hm = amp * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8.0)
    return (hm + 0.02 * torch.rand((n, 17, H, W), device="cuda", generator=g)).contiguous()


def _geometry(g, n):
    center = (g.uniform(0.1, 0.9, size=(n, 2)) * np.array([W_PX, H_PX])).astype(np.float32)
    scale = (g.uniform(0.8, 2.5, size=(n, 1)) * np.array([0.75, 1.0])).astype(np.float32)
    return torch.from_numpy(center).cuda(), torch.from_numpy(scale).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    g = np.random.default_rng(args.seed)
    lib = _lib.load()
    res = {"what": "heatmaps in, keypoints out (measured; CUDA events for the device, host clock for the host path, median of %d)" % args.reps,
           "maps": [17, H, W], "device": torch.cuda.get_device_name(0)}

    decode, host = {}, {}
    for n in (22, 1024):
        hm32 = _maps(args.seed + n, n)
        center, scale = _geometry(g, n)
        geom = torch.cat((center, scale), dim=-1).contiguous()
        out, scratch = torch.empty((n, 17, 3), device="cuda"), torch.empty((n, 17, 3), device="cuda")
        for name, hm, code in (("fp32", hm32, _lib.DTYPE_F32), ("fp16", hm32.half(), _lib.DTYPE_F16)):
            layouts = (("coco", _lib.LAYOUT_COCO), ("h36m", _lib.LAYOUT_H36M)) if n == 22 else (("coco", _lib.LAYOUT_COCO),)
            for lname, layout in layouts:
                def launch():
                    return lib.kasf_heatmap_keypoints(hm.data_ptr(), code, n, H, W, geom.data_ptr(), _lib.GEOM_CENTER_SCALE, 1.0, 1, layout, out.data_ptr(),
                                                      scratch.data_ptr(), stream())
                for _ in range(3):
                    _lib.check(launch())
                reps = []
                for _ in range(args.reps):
                    _, e, _ = _timed(lambda: [_lib.check(launch()) for _ in range(args.kernel_iters)])
                    reps.append(e / args.kernel_iters)
                ms = statistics.median(reps)
                nbytes = hm.numel() * hm.element_size() + geom.numel() * 4 + out.numel() * 4 * (3 if layout == _lib.LAYOUT_H36M else 1)
                decode[f"{name} {lname} @ n={n}"] = {"us": round(ms * 1e3, 2), "min_us": round(min(reps) * 1e3, 2), "GB_per_s": round(nbytes / ms / 1e6, 1)}
        # the host path: D2H copy + numpy, from the same device tensor
        c_h, s_h = center.cpu().numpy(), scale.cpu().numpy()
        want = K.heatmaps_to_keypoints(hm32, center, scale).cpu()
        copy_ms, numpy_ms, total_ms = [], [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            on_host = hm32.clone().cpu().numpy()
            t1 = time.perf_counter()
            got = heatmap_decode_np(on_host, c_h, s_h)
            t2 = time.perf_counter()
            copy_ms.append((t1 - t0) * 1e3)
            numpy_ms.append((t2 - t1) * 1e3)
            total_ms.append((t2 - t0) * 1e3)
        host[f"fp32 @ n={n}"] = {"d2h_copy_ms": round(statistics.median(copy_ms), 4), "numpy_decode_ms": round(statistics.median(numpy_ms), 4),
                                 "total_ms": round(statistics.median(total_ms), 4), "equal_to_device": bool(torch.equal(torch.from_numpy(got), want))}
        # ... and the device path as a caller sees it (Python surface, host clock up to a synchronise)
        K.heatmaps_to_keypoints(hm32, center, scale)
        wall = [_timed(lambda: K.heatmaps_to_keypoints(hm32, center, scale))[2] for _ in range(args.reps)]
        host[f"fp32 @ n={n}"]["device_call_wall_ms"] = round(statistics.median(wall), 4)
        del hm32
    res["decode_kernel"], res["host_path"] = decode, host

    # the live tick
    model = K.KASportsFormer(n_layers=args.layers, num_heads=8, n_frames=T, compute_dtype=args.dtype).cuda().eval()
    res.update(layers=args.layers, dtype=args.dtype, T=T)
    S, n = 22, args.warmup + args.ticks
    pool = [_maps(args.seed + 5000 + i, S) for i in range(8)]   # 8 different ticks of heatmaps, cycled
    center, scale = _geometry(g, S)
    ready = [K.heatmaps_to_keypoints(hm, center, scale, layout="h36m") for hm in pool]
    from_maps, from_kp = K.StreamLifter(model, W_PX, H_PX, slots=S), K.StreamLifter(model, W_PX, H_PX, slots=S)
    ms = {"push_heatmaps": [], "push_ready_keypoints": []}
    same = True
    for i in range(n):
        a, e_a, _ = _timed(lambda: from_maps.push_heatmaps(pool[i % 8], center, scale))
        b, e_b, _ = _timed(lambda: from_kp.push(ready[i % 8]))
        same = same and bool(torch.equal(a, b))
        if i >= args.warmup:
            ms["push_heatmaps"].append(e_a)
            ms["push_ready_keypoints"].append(e_b)
    res["stream_22_slots_event_ms"] = {k: _stats(v) for k, v in ms.items()}
    res["stream_22_slots_event_ms"]["poses_equal"] = same
    print(json.dumps(res))


if __name__ == "__main__":
    main()
