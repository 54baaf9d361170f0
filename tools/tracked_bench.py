#!/usr/bin/env python3
"""The seam between the tracker and the lift: SortTracker.update -> TrackedLifter.push per tick against what a caller did before TrackedLifter existed,
SortTracker.update, a read-back of ids / slot / born / count, StreamLifter.reset and push(slots=...) decided on the host.

    python tools/tracked_bench.py [--persons 2 22] [--layers 26] [--dtype bf16] [--ticks 200] [--warmup 40] [--kernel-iters 20] [--seed 0]

One stream, the shipped model (26 layers, 8 heads, T = 27, bf16; random weights, which the time does not depend on), flip-TTA on, lag 0; seeded boxes of
--persons people drifting over a 1280 x 720 frame and seeded keypoints, all on the device before timing; two trackers fed the same boxes, 32 slots.  After
--warmup ticks of both ways (rings full from tick T on), --ticks ticks, each running (a) the device path and (b) the read-back path, alternating within the
tick; each timed with CUDA events and with the host clock up to a synchronise.  Reports median and 99th percentile per tick of both, whether their poses were
equal, and kasf_stream_track_front alone against kasf_stream_push + kasf_stream_windows for the same rows: events around --kernel-iters back-to-back
launches, per launch.  Prints one JSON line per --persons value.
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

T, W_PX, H_PX, SLOTS = 27, 1280, 720, 32


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


def _boxes(g, n, P):
    """[n, 1, P, 5] boxes of P people on a grid, each drifting a little per tick: x1, y1, x2, y2, score."""
    cols = int(np.ceil(np.sqrt(P * W_PX / H_PX)))
    rows = int(np.ceil(P / cols))
    cx = (np.arange(P) % cols + 0.5) * W_PX / cols
    cy = (np.arange(P) // cols + 0.5) * H_PX / rows
    w, h = 0.45 * W_PX / cols, 0.8 * H_PX / rows
    drift = np.cumsum(g.normal(0, 0.5, size=(n, P, 2)), axis=0)
    c = np.stack((cx, cy), axis=-1)[None] + drift
    out = np.concatenate((c - (w / 2, h / 2), c + (w / 2, h / 2), np.full((n, P, 1), 0.9)), axis=-1)
    return out[:, None].astype(np.float32)


def run(P, args):
    n = args.warmup + args.ticks
    g = np.random.default_rng(args.seed)
    boxes = torch.from_numpy(_boxes(g, n, P)).cuda()
    count = torch.full((1,), P, dtype=torch.int32, device="cuda")
    kps = torch.from_numpy(np.concatenate((g.uniform((0, 0), (W_PX, H_PX), size=(n, P, 17, 2)), g.uniform(0.3, 1, size=(n, P, 17, 1))),
                                          axis=-1).astype(np.float32)).cuda()
    model = K.KASportsFormer(n_layers=args.layers, num_heads=8, n_frames=T, compute_dtype=args.dtype).cuda().eval()
    trk_a, trk_b = (K.SortTracker(streams=1, slots=SLOTS, min_hits=0, num_person=P, hold_last=True) for _ in range(2))
    tracked = K.TrackedLifter(model, W_PX, H_PX, streams=1, track_slots=SLOTS, rows="persons", num_person=P, flip=True, lag=0)
    plain = K.StreamLifter(model, W_PX, H_PX, slots=SLOTS, flip=True, lag=0)
    holder = {}

    def device_path(t):
        return tracked.push(kps[t], trk_a.update(boxes[t], count)).poses[0]

    def read_back_path(t):
        r = trk_b.update(boxes[t], count)
        ids, slot, born, c = r.ids[0].cpu().tolist(), r.slot[0].cpu().tolist(), r.born[0].cpu().tolist(), int(r.count[0])
        rows = [c - 1 - k for k in range(min(c, P))]
        fresh = [slot[q] for q in rows if holder.get(slot[q]) != ids[q] or born[q]]
        if fresh:
            plain.reset(slots=fresh)
        for q in rows:
            holder[slot[q]] = ids[q]
        out = torch.zeros((P, 17, 3), device="cuda")
        if rows:
            out[:len(rows)] = plain.push(kps[t][:len(rows)], slots=[slot[q] for q in rows])
        return out

    ms, wall = {"tracked": [], "read_back": []}, {"tracked": [], "read_back": []}
    equal = True
    for t in range(n):
        got, e_a, w_a = _timed(lambda: device_path(t))
        ref, e_b, w_b = _timed(lambda: read_back_path(t))
        equal = equal and bool(torch.equal(got, ref))
        if t >= args.warmup:
            ms["tracked"].append(e_a)
            wall["tracked"].append(w_a)
            ms["read_back"].append(e_b)
            wall["read_back"].append(w_b)

    lib = _lib.load()
    r = trk_a.update(boxes[n - 1], count)
    frame = kps[0]
    x = torch.empty((2 * P, T, 17, 3), device="cuda")
    row_slot = torch.empty(P, dtype=torch.int32, device="cuda")
    ring, cnt, owner = tracked._ring.clone(), tracked._count.clone(), tracked._owner.clone()
    ring_p, cnt_p = plain._ring.clone(), plain._count.clone()
    ids_d = torch.arange(P, dtype=torch.int32, device="cuda")
    launches = {
        "stream_track_front": lambda: lib.kasf_stream_track_front(frame.data_ptr(), r.ids.data_ptr(), r.slot.data_ptr(), r.born.data_ptr(), r.count.data_ptr(), 1,
                                                                  SLOTS, 0, P, T, ring.data_ptr(), cnt.data_ptr(), owner.data_ptr(), tracked._width.data_ptr(),
                                                                  tracked._height.data_ptr(), tracked._r_tab.data_ptr(), 1, x.data_ptr(), row_slot.data_ptr(),
                                                                  stream()),
        "stream_push": lambda: lib.kasf_stream_push(frame.data_ptr(), ids_d.data_ptr(), P, SLOTS, T, ring_p.data_ptr(), cnt_p.data_ptr(), stream()),
        "stream_windows": lambda: lib.kasf_stream_windows(ring_p.data_ptr(), cnt_p.data_ptr(), ids_d.data_ptr(), P, SLOTS, T, plain._width.data_ptr(),
                                                          plain._height.data_ptr(), plain._r_tab.data_ptr(), 1, x.data_ptr(), stream()),
    }
    kernel_ms = {}
    for name, launch in launches.items():
        _lib.check(launch())
        reps = []
        for _ in range(args.reps):
            _, e, _ = _timed(lambda: [_lib.check(launch()) for _ in range(args.kernel_iters)])
            reps.append(e / args.kernel_iters)
        kernel_ms[name] = round(statistics.median(reps), 5)
    print(json.dumps({"what": "tracker -> lift per tick: SortTracker.update + TrackedLifter.push vs update + read-back + StreamLifter.reset / push(slots=) "
                              "(measured, %d ticks after %d warm-up)" % (args.ticks, args.warmup),
                      "streams": 1, "persons": P, "track_slots": SLOTS, "clips_per_tick": 2 * P, "T": T, "layers": args.layers, "dtype": args.dtype, "lag": 0,
                      "event_ms": {k: _stats(v) for k, v in ms.items()}, "wall_ms": {k: _stats(v) for k, v in wall.items()},
                      "wall_median_ratio_read_back_over_tracked": round(statistics.median(wall["read_back"]) / statistics.median(wall["tracked"]), 3),
                      "kernel_ms_per_launch": kernel_ms, "poses_equal": equal, "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, nargs="+", default=[2, 22])
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5, help="repetitions of the kernel-alone timings")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.warmup < T:
        ap.error(f"--warmup must be at least T = {T}: both ways are timed on full windows")
    if not torch.cuda.is_available():
        sys.exit("tracked_bench: needs a GPU; there is no CPU path to time")
    for P in args.persons:
        if not 1 <= P <= SLOTS:
            ap.error(f"--persons must be in [1, {SLOTS}]")
        run(P, args)


if __name__ == "__main__":
    main()
