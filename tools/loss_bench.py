#!/usr/bin/env python3
"""The seven-term training loss alone on the device: kasf_loss7 with all six lambdas set, with only the three old ones set, kasf_loss3, and the eager-torch path
kasf_loss7 replaces.

    python tools/loss_bench.py [--reps 7] [--kernel-iters 50] [--eager-iters 5] [--seed 0] [--step-timeout 180] [--out FILE.json]

Seeded clips on the device (target ~ 0.3 N(0,1), pred = target + 0.05 N(0,1)) at B = 256, T = 27 (the benchmark's step) and B = 32, T = 243.  One step per shape,
each a child process of its own under its own time limit (--step-timeout seconds); the first step that fails, faults or runs out of time ends the run, nothing is
started after it.  Per step, all in one process and timed the same way (three warm-up rounds, then CUDA events around back-to-back rounds, per round, median and
minimum of --reps):
  loss7_all   kasf_loss7 (both launches), lambdas 0.5, 20, 0.5, 0.25, 0.1, 0.2: every term's gradient
  loss7_old3  kasf_loss7 with the four new lambdas 0: all seven parts, the three old terms' gradient
  loss3       kasf_loss3 (both launches)
  eager       a RESTATEMENT of the reference's seven formulas in fp32 torch on the device (tests/loss_ref.py, the one the tests tie to utils/loss_calc.py) plus
              .backward(): what a caller had to run before; --eager-iters rounds
  ratios      loss7_all over loss3, loss7_old3 over loss3, eager over loss7_all
Prints one JSON line; --out also writes it to a file (stamp it with tools/stamp.py --embed).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"b256_t27": (256, 27), "b32_t243": (32, 243)}
ALL = (0.5, 20.0, 0.5, 0.25, 0.1, 0.2)
OLD3 = (0.5, 20.0, 0.0, 0.0, 0.0, 0.0)


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


def step_shape(args, name):
    import torch
    from kasportsformer_amd import _lib
    from tests.loss_ref import parts7
    lib = _lib.load()
    B, T = STEPS[name]
    g = torch.Generator(device="cuda").manual_seed(args.seed + B)
    target = 0.3 * torch.randn((B, T, 17, 3), generator=g, device="cuda")
    pred = target + 0.05 * torch.randn((B, T, 17, 3), generator=g, device="cuda")
    dpred = torch.empty_like(pred)
    losses7, losses3 = torch.empty(8 + 8 * B, device="cuda"), torch.empty(4 + 4 * B, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lam_all, lam_old = (C.c_float * 6)(*ALL), (C.c_float * 6)(*OLD3)

    def loss7(lam):
        _lib.check(lib.kasf_loss7(pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), losses7.data_ptr(), losses7.numel(), B, T, lam, 1.0, stream))

    def loss3():
        _lib.check(lib.kasf_loss3(pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), losses3.data_ptr(), losses3.numel(), B, T, 0.5, 20.0, 1.0, stream))

    leaf = pred.clone().requires_grad_(True)

    def eager():
        leaf.grad = None
        parts = parts7(leaf, target)
        total = parts[0]
        for lam, part in zip(ALL, parts[1:]):
            total = total + lam * part
        total.backward()
        return total

    t = {"loss7_all": _per_round(lambda: loss7(lam_all), args.reps, args.kernel_iters), "loss7_old3": _per_round(lambda: loss7(lam_old), args.reps, args.kernel_iters),
         "loss3": _per_round(loss3, args.reps, args.kernel_iters), "eager": _per_round(eager, args.reps, args.eager_iters)}
    loss7(lam_all)
    total = eager()
    torch.cuda.synchronize()
    row = {k: {"us": round(med * 1e3, 2), "min_us": round(best * 1e3, 2)} for k, (med, best) in t.items()}
    row["ratios"] = {"loss7_all over loss3": round(t["loss7_all"][0] / t["loss3"][0], 3), "loss7_old3 over loss3": round(t["loss7_old3"][0] / t["loss3"][0], 3),
                     "eager over loss7_all": round(t["eager"][0] / t["loss7_all"][0], 3)}
    row["total"] = {"loss7": float(losses7[0]), "eager": float(total)}
    row["gradient max |loss7 - eager| / max |eager|"] = float((dpred - leaf.grad).abs().max() / leaf.grad.abs().max())
    row["device"] = torch.cuda.get_device_name(0)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--eager-iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_shape(args, args.step)))
        return 0
    res = {"what": "seven-term loss: kasf_loss7 with every lambda set, with the three old ones only, kasf_loss3, and the eager-torch restatement it replaces "
                   "(measured; CUDA events, median of %d)" % args.reps}
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
