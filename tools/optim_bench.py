#!/usr/bin/env python3
"""The optimiser step of the 26-layer model alone, and the whole training step with each optimiser.

    python tools/optim_bench.py [--reps 21] [--iters 10] [--train-steps 10] [--batch 256] [--step-timeout 300] [--out FILE.json]

One case per child process, each under its own time limit (--step-timeout seconds); the first case that fails, faults or runs out of time ends the run, nothing
is started after it.  The parent never opens the GPU.

The step alone (n_layers=26, T=27; one backward of four clips leaves the gradients, every step then reads the same ones).  Per case three warm-up steps, then
--reps rounds of --iters back-to-back steps; `device_us` is the CUDA-event time per step, `host_us` the host clock around the same calls without a
synchronisation in between (what the Python side of step() costs the training loop), median and minimum over the rounds; where step() is host-bound the two
agree, and `kernels_us` (the K optimisers) is the CUDA-event time of the step's launches re-issued back to back without step()'s host work:
  stock              torch.optim.AdamW(model.parameters())           the foreach update over the views of the flat array (INTEGRATION.md path A)
  stock_fused        the same with fused=True
  fused              K.FusedAdamW(model)                             one launch over [0, n_live)
  kadamw             K.AdamW(model.parameters())                     one launch over the chunk table
  kadamw_clip        ... with max_grad_norm=1.0                      two more launches in front
  kadamw_two_groups  K.AdamW over a no-decay group (1-D tensors, position embeddings) and the rest

The whole training step (forward, zero_grad, loss3, backward, step) at B = --batch, T = 27, bf16: clips/s from the host clock around --train-steps steps between
two synchronisations, median of --reps rounds:
  train_stock        path A with the stock optimiser
  train_kadamw       path A with K.AdamW: the one-token change
  train_fused        K.FusedAdamW with attach_param_grads = False (the benchmark's path)
Prints one JSON line; --out also writes it to a file.
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

STEP_CASES = ("stock", "stock_fused", "fused", "kadamw", "kadamw_clip", "kadamw_two_groups")
TRAIN_CASES = ("train_stock", "train_kadamw", "train_fused")
LR, WD = 5e-4, 0.01


def no_decay_groups(model):
    names = {id(p): n for n, p in model.named_parameters()}
    plain = [p for p in model.parameters() if p.dim() == 1 or names[id(p)].endswith("pos_embed")]
    ids = {id(p) for p in plain}
    return [{"params": plain, "weight_decay": 0.0}, {"params": [p for p in model.parameters() if id(p) not in ids]}]


def make_optimizer(K, torch, model, case):
    kind = case.replace("train_", "")
    if kind == "stock":
        return torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    if kind == "stock_fused":
        return torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD, fused=True)
    if kind == "fused":
        return K.FusedAdamW(model, lr=LR, weight_decay=WD)
    if kind == "kadamw":
        return K.AdamW(model.parameters(), lr=LR, weight_decay=WD)
    if kind == "kadamw_clip":
        return K.AdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=1.0)
    return K.AdamW(no_decay_groups(model), lr=LR, weight_decay=WD)


def run_case(args, case):
    import torch
    import kasportsformer_amd as K
    model = K.KASportsFormer(n_layers=26, n_frames=27, compute_dtype="bf16").cuda().train()
    opt = make_optimizer(K, torch, model, case)
    row = {"device": torch.cuda.get_device_name(0), "parameters": sum(1 for _ in model.parameters()), "n_live": model.n_live}
    if case in STEP_CASES:
        x, y = (t.cuda() for t in K.synthetic_clips(4, 27, seed=args.seed))
        K.loss3(model(x), y)[0].backward()
        for _ in range(3):
            opt.step()
        dev, host = [], []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                opt.step()
            t1 = time.perf_counter()
            b.record()
            torch.cuda.synchronize()
            dev.append(a.elapsed_time(b) * 1e3 / args.iters)
            host.append((t1 - t0) * 1e6 / args.iters)
        row.update(device_us=round(statistics.median(dev), 1), device_min_us=round(min(dev), 1), host_us=round(statistics.median(host), 1),
                   host_min_us=round(min(host), 1))
        if case.startswith("kadamw"):
            row.update(chunks=opt._table[1], launches=len(opt._launches) + (2 if opt.max_grad_norm is not None else 0))
        # the launches alone, without step()'s host work in between: what the kernels take when the host keeps the queue full
        if case == "fused":
            replay = opt.step
        elif case.startswith("kadamw"):
            seen, launch = [], opt._launch
            opt._launch = lambda *a: (seen.append(a), launch(*a))
            opt.step()
            opt._launch = launch
            replay = lambda: launch(*seen[0])
        else:
            return row
        ker = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.iters):
                replay()
            b.record()
            torch.cuda.synchronize()
            ker.append(a.elapsed_time(b) * 1e3 / args.iters)
        row.update(kernels_us=round(statistics.median(ker), 1), kernels_min_us=round(min(ker), 1))
        return row
    if case == "train_fused":
        model.attach_param_grads = False
    x, y = (t.cuda() for t in K.synthetic_clips(args.batch, 27, seed=args.seed))

    def step():
        pred = model(x)
        opt.zero_grad()
        K.loss3(pred, y)[0].backward()
        opt.step()

    for _ in range(3):
        step()
    rates = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.train_steps):
            step()
        torch.cuda.synchronize()
        rates.append(args.batch * args.train_steps / (time.perf_counter() - t0))
    row.update(clips_per_s=round(statistics.median(rates), 1), clips_per_s_max=round(max(rates), 1), batch=args.batch)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--cases", default=",".join(STEP_CASES + TRAIN_CASES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", choices=STEP_CASES + TRAIN_CASES, default=None, help="run one case in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: a median of at least 20")
    if args.case:
        print(json.dumps(run_case(args, args.case)))
        return 0
    res = {"what": "optimiser step alone (26 layers; CUDA events and host clock per step) and the whole bf16 training step in clips/s, per optimiser "
                   "(measured; median of %d)" % args.reps}
    code = 0
    for case in args.cases.split(","):                       # each case is a fresh process under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps), "--iters", str(args.iters), "--train-steps",
               str(args.train_steps), "--batch", str(args.batch), "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            res[case] = {"failed": f"no result within {args.step_timeout} s"}
            code = 1
            break
        if r.returncode != 0:
            res[case] = {"failed": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            code = 1
            break
        res[case] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return code


if __name__ == "__main__":
    sys.exit(main())
