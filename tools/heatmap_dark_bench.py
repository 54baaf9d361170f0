#!/usr/bin/env python3
"""Pose-network heatmaps in, DARK / DARK-UDP keypoints out: kasf_heatmap_decode alone on the device in modes 1 and 2, plain and flip-tested, against the existing
quarter-pixel entries over the same bytes.

    python tools/heatmap_dark_bench.py [--reps 7] [--kernel-iters 50] [--kernel 11] [--seed 0] [--step-timeout 180] [--out FILE.json]

22 and 1,024 persons of 17 x 96 x 72 maps of seeded noise on the device, in fp32 and fp16.  One step per dtype, each a child process of its own under its own
time limit (--step-timeout seconds); the first step that fails, faults or runs out of time ends the run, nothing is started after it.  Per step and size, all
in one process and timed the same way (three warm-up rounds, then CUDA events around --kernel-iters back-to-back launches, per launch, median and minimum of
--reps), with GB/s of bytes READ (each array once):
  quarter, flip quarter        kasf_heatmap_keypoints / kasf_heatmap_flip_keypoints: the yardsticks
  dark, dark_udp               kasf_heatmap_decode, modes 1 and 2, --kernel taps, no flip test
  flip dark, flip dark_udp     the same with the flip test (shift on, COCO pairs, no merged output)
  decode quarter               kasf_heatmap_decode in mode 0 without udp: the new kernels' streaming pass and finish alone
  ratios                       each new launch over its yardstick.  None is a pass / fail bar.
Prints one JSON line; --out also writes it to a file (stamp it with tools/stamp.py --embed).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 96, 72
PERSONS = (22, 1024)
STEPS = ("fp32", "fp16")


def _per_round(fn, reps, iters):
    """(median, minimum) ms per call of fn(): three warm-up calls, then CUDA events around `iters` back-to-back calls, `reps` times."""
    import torch
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return statistics.median(ms), min(ms)


def step_dtype(args, name):
    import torch
    from kasportsformer_amd import _lib, gaussian_weights
    from kasportsformer_amd._args import DTYPES, stream
    from kasportsformer_amd.heatmap import partner_table
    lib = _lib.load()
    dtype = {"fp32": torch.float32, "fp16": torch.float16}[name]
    code, size = DTYPES[dtype], torch.empty((), dtype=dtype).element_size()
    partner = partner_table(None, "heatmap_dark_bench")
    weights = gaussian_weights(args.kernel)
    res = {"device": torch.cuda.get_device_name(0)}
    for n in PERSONS:
        g = torch.Generator(device="cuda").manual_seed(args.seed + n)
        hm, hmf = (torch.randn((n, 17, H, W), generator=g, device="cuda").to(dtype) for _ in range(2))
        geom = torch.tensor([[600.0, 350.0, 1.5, 2.0]] * n, device="cuda")
        out = torch.empty((n, 17, 3), device="cuda")

        def quarter():
            _lib.check(lib.kasf_heatmap_keypoints(hm.data_ptr(), code, n, H, W, geom.data_ptr(), _lib.GEOM_CENTER_SCALE, 1.0, 1, _lib.LAYOUT_COCO, out.data_ptr(),
                                                  None, stream()))

        def flip_quarter():
            _lib.check(lib.kasf_heatmap_flip_keypoints(hm.data_ptr(), hmf.data_ptr(), code, n, H, W, partner.ctypes.data, 1, geom.data_ptr(), _lib.GEOM_CENTER_SCALE,
                                                       1.0, 1, _lib.LAYOUT_COCO, out.data_ptr(), None, None, stream()))

        def decode(mode, flipped):
            def run():
                _lib.check(lib.kasf_heatmap_decode(hm.data_ptr(), hmf.data_ptr() if flipped else None, code, n, H, W, partner.ctypes.data if flipped else None, 1,
                                                   geom.data_ptr(), _lib.GEOM_CENTER_SCALE, 1.0, mode, weights.ctypes.data, args.kernel,
                                                   int(mode == _lib.DECODE_DARK_UDP), _lib.LAYOUT_COCO, out.data_ptr(), None, None, stream()))
            return run

        runs = {"quarter": (quarter, 1), "flip quarter": (flip_quarter, 2), "decode quarter": (decode(_lib.DECODE_QUARTER, False), 1),
                "dark": (decode(_lib.DECODE_DARK, False), 1), "dark_udp": (decode(_lib.DECODE_DARK_UDP, False), 1),
                "flip dark": (decode(_lib.DECODE_DARK, True), 2), "flip dark_udp": (decode(_lib.DECODE_DARK_UDP, True), 2)}
        t = {k: _per_round(fn, args.reps, args.kernel_iters) for k, (fn, _) in runs.items()}
        one = n * 17 * H * W * size
        row = {k: {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2), "MB": round(runs[k][1] * one / 1e6, 2),
                   "GB_per_s": round(runs[k][1] * one / med / 1e6, 1)} for k, (med, best) in t.items()}
        row["ratios"] = {f"{k} over {y}": round(t[k][0] / t[y][0], 3) for k, y in (("decode quarter", "quarter"), ("dark", "quarter"), ("dark_udp", "quarter"),
                                                                                   ("flip dark", "flip quarter"), ("flip dark_udp", "flip quarter"))}
        res[f"{n} persons"] = row
        del hm, hmf
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--kernel", type=int, default=11, help="taps of the Gaussian (odd, 1..17)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_dtype(args, args.step)))
        return 0
    res = {"what": "DARK / DARK-UDP heatmap decode: kasf_heatmap_decode against the quarter-pixel entries over the same bytes (measured; CUDA events, median of %d)"
                   % args.reps, "maps": [17, H, W], "kernel": args.kernel}
    code = 0
    for step in STEPS:                                       # the parent never opens the GPU: each step is a fresh process under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--kernel-iters", str(args.kernel_iters),
               "--kernel", str(args.kernel), "--seed", str(args.seed)]
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
