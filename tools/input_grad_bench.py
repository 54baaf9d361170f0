#!/usr/bin/env python3
"""What the gradient with respect to the input keypoints costs: one training step with and without x.requires_grad, and kasf_op_input_grad alone.

    python tools/input_grad_bench.py [--reps 9] [--op-iters 50] [--seed 0] [--step-timeout 420] [--out FILE.json]

Two steps, each a child process of its own under its own time limit (--step-timeout seconds); the first step that fails, faults or runs out of time ends the
run, nothing is started after it.
  train_step  the 26-layer bf16 model at B = 256, T = 27 (the benchmark's step): forward, kasf_loss3, backward, FusedAdamW.  Two arms in ONE process, alternating
              round by round (three warm-up rounds each): x as it is, and x.requires_grad_() -- three more workspace entries, two more din3 stores in the
              embedding backward, one k_input_grad launch, one clone of dx.  CUDA events around every step; median and minimum of --reps, and the median of the
              per-round differences.
  op          kasf_op_input_grad alone at 6,912 frames (= 256 x 27), all three gradients given: CUDA events around --op-iters back-to-back calls, per call,
              median and minimum of --reps.
There is no pass bar.  Prints one JSON line; --out also writes it to a file (stamp it with tools/stamp.py --embed).
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

STEPS = ("train_step", "op")
B, T, LAYERS = 256, 27, 26


def step_train(args):
    import torch
    import kasportsformer_amd as K
    torch.manual_seed(114514)
    m = K.KASportsFormer(n_layers=LAYERS, num_heads=8, n_frames=T, compute_dtype="bf16").cuda().train()
    m.attach_param_grads = False
    opt = K.FusedAdamW(m, lr=5e-4, weight_decay=0.01)
    x, y = (t.cuda() for t in K.synthetic_clips(B, T, seed=1234 + args.seed))

    def step(req):
        xin = x.clone().requires_grad_(req)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        opt.zero_grad()
        loss, _ = K.loss3(m(xin), y)
        loss.backward()
        opt.step()
        b.record()
        torch.cuda.synchronize()
        assert (xin.grad is not None) == req
        return a.elapsed_time(b)

    for _ in range(3):
        step(False)
        step(True)
    ms = {False: [], True: []}
    for _ in range(args.reps):
        for req in (False, True):
            ms[req].append(step(req))
    diff = [w - wo for w, wo in zip(ms[True], ms[False])]
    row = {name: {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "clips_per_s": round(B * 1e3 / statistics.median(v), 1)}
           for name, v in (("without", ms[False]), ("with_x_grad", ms[True]))}
    row["median of per-round differences, ms"] = round(statistics.median(diff), 3)
    row["with over without"] = round(statistics.median(ms[True]) / statistics.median(ms[False]), 4)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def step_op(args):
    import torch
    from kasportsformer_amd import _lib
    lib = _lib.load()
    frames = B * T
    cfg, h = _lib.KasfConfig(1, T, 8, 4, 1, 1), C.c_void_p()
    _lib.check(lib.kasf_model_create(C.byref(cfg), C.byref(h)))
    g = torch.Generator(device="cuda").manual_seed(args.seed)
    params = 0.3 * torch.randn(lib.kasf_param_count(h), generator=g, device="cuda")
    x = torch.rand((frames, 17, 3), generator=g, device="cuda") * 2 - 1
    grads = [torch.randn((frames, 17, 3), generator=g, device="cuda") for _ in range(3)]
    dx = torch.empty_like(x)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.kasf_op_input_grad(h, params.data_ptr(), x.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), dx.data_ptr(),
                                          frames, stream))

    for _ in range(3):
        call()
    us = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.op_iters):
            call()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / args.op_iters)
    ok = bool(torch.isfinite(dx).all())
    torch.cuda.synchronize()
    lib.kasf_model_destroy(h)
    return {"frames": frames, "us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "finite": ok, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=STEPS, default=None, help="run one step in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"train_step": step_train, "op": step_op}[args.step](args)))
        return 0
    res = {"what": "gradient with respect to the input keypoints: the training step at B = %d, T = %d (26 layers, bf16) with and without x.requires_grad, and "
                   "kasf_op_input_grad alone (measured; CUDA events, median of %d)" % (B, T, args.reps)}
    code = 0
    for step in STEPS:                                       # the parent never opens the GPU: each step is a fresh process under its own time limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--op-iters", str(args.op_iters), "--seed", str(args.seed)]
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
