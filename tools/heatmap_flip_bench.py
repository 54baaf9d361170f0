#!/usr/bin/env python3
"""Two heatmap arrays in (the pose network's output for the crops and for the mirrored crops), flip-tested keypoints out: kasf_heatmap_flip_keypoints alone on
the device, its yardstick, and the eager-torch path it replaces.

    python tools/heatmap_flip_bench.py [--reps 7] [--kernel-iters 50] [--eager-iters 10] [--seed 0] [--step-timeout 180] [--out FILE.json]

22 and 1,024 persons of 17 x 96 x 72 maps of seeded noise on the device, in fp32 and fp16.  One step per dtype, each a child process of its own under its own
time limit (--step-timeout seconds); the first step that fails, faults or runs out of time ends the run, nothing is started after it.  Per step and size, all
in one process and timed the same way (three warm-up rounds, then CUDA events around back-to-back rounds, per round, median and minimum of --reps):
  flip       the new launch alone (shift on, COCO pairs, refine on, no merged output), --kernel-iters launches, with GB/s of bytes READ (both arrays once)
  merged     the same launch with the fp32 merged maps stored as well (GB/s of bytes read + written)
  yardstick  two kasf_heatmap_keypoints launches, one over each array: the same bytes read, no flip, no merge
  eager      what a caller had to do before: flip(-1), the index gather over the joint axis, the slice copy for the shift, add, multiply -- in the tensors' own
             dtype, which for fp16 is NOT the float32 rule of the new entry -- and kasf_heatmap_keypoints on the result; --eager-iters rounds
  ratios     flip over yardstick, eager over flip, eager over yardstick
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
    import numpy as np
    import torch
    from kasportsformer_amd import _lib
    from kasportsformer_amd._args import DTYPES, stream
    from kasportsformer_amd.heatmap import partner_table
    lib = _lib.load()
    dtype = {"fp32": torch.float32, "fp16": torch.float16}[name]
    code, size = DTYPES[dtype], torch.empty((), dtype=dtype).element_size()
    partner = partner_table(None, "heatmap_flip_bench")
    partner_d = torch.from_numpy(partner.astype(np.int64)).cuda()
    res = {"device": torch.cuda.get_device_name(0)}
    for n in PERSONS:
        g = torch.Generator(device="cuda").manual_seed(args.seed + n)
        hm, hmf = (torch.randn((n, 17, H, W), generator=g, device="cuda").to(dtype) for _ in range(2))
        geom = torch.tensor([[600.0, 350.0, 1.5, 2.0]] * n, device="cuda")
        out, out2 = torch.empty((n, 17, 3), device="cuda"), torch.empty((n, 17, 3), device="cuda")
        merged = torch.empty((n, 17, H, W), device="cuda")

        def flip(store=None):
            _lib.check(lib.kasf_heatmap_flip_keypoints(hm.data_ptr(), hmf.data_ptr(), code, n, H, W, partner.ctypes.data, 1, geom.data_ptr(), _lib.GEOM_CENTER_SCALE,
                                                       1.0, 1, _lib.LAYOUT_COCO, out.data_ptr(), None, store, stream()))

        def decode(t, o):
            _lib.check(lib.kasf_heatmap_keypoints(t.data_ptr(), DTYPES[t.dtype], n, H, W, geom.data_ptr(), _lib.GEOM_CENTER_SCALE, 1.0, 1, _lib.LAYOUT_COCO,
                                                  o.data_ptr(), None, stream()))

        def yardstick():
            decode(hm, out2)
            decode(hmf, out2)

        def eager():
            back = hmf.flip(-1)[:, partner_d]
            shifted = back.clone()
            shifted[..., 1:] = back[..., :-1]
            decode((hm + shifted) * 0.5, out2)

        read = 2 * n * 17 * H * W * size
        t = {"flip": _per_round(flip, args.reps, args.kernel_iters), "merged": _per_round(lambda: flip(merged.data_ptr()), args.reps, args.kernel_iters),
             "yardstick": _per_round(yardstick, args.reps, args.kernel_iters), "eager": _per_round(eager, args.reps, args.eager_iters)}
        eager()
        flip()
        torch.cuda.synchronize()
        moved = {"flip": read, "merged": read + n * 17 * H * W * 4, "yardstick": read}
        row = {k: {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2),
                   **({"MB": round(moved[k] / 1e6, 2), "GB_per_s": round(moved[k] / med / 1e6, 1)} if k in moved else {})} for k, (med, best) in t.items()}
        row["ratios"] = {"flip over yardstick": round(t["flip"][0] / t["yardstick"][0], 3), "eager over flip": round(t["eager"][0] / t["flip"][0], 3),
                         "eager over yardstick": round(t["eager"][0] / t["yardstick"][0], 3)}
        row["eager_equal_to_flip"] = bool(torch.equal(out, out2))          # expected for fp32 only: fp16 eager arithmetic rounds the sum to half
        res[f"{n} persons"] = row
        del hm, hmf, merged
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--eager-iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_dtype(args, args.step)))
        return 0
    res = {"what": "flip-tested heatmap decode: the new launch, two plain decodes over the same bytes, and the eager-torch path (measured; CUDA events, median of %d)"
                   % args.reps, "maps": [17, H, W]}
    code = 0
    for step in STEPS:                                       # the parent never opens the GPU: each step is a fresh process under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--kernel-iters", str(args.kernel_iters),
               "--eager-iters", str(args.eager_iters), "--seed", str(args.seed)]
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
