#!/usr/bin/env python3
"""The One-Euro filter on the device (kasportsformer_amd.OneEuroFilter / smooth_tracks) against what a caller would do without it.

    python tools/smooth_bench.py [--steps launches host tick] [--persons 2 22] [--layers 26] [--dtype bf16] [--ticks 100] [--warmup 30] [--iters 50] [--reps 5]

Every step runs in a child process of its own under its own time limit, one after the other; a step that fails or runs out of time ends the run.
  launches  kasf_one_euro_push and kasf_one_euro_tracked alone at 22 and 1,024 rows of 17 x (x, y, score), kasf_one_euro_tracks at one 18,000-frame track:
            CUDA events around --iters back-to-back launches (the tick advancing, so every launch updates), per launch, the median of --reps.
  host      the path they replace, for the same inputs: download of the keypoints (and of ids / slot / born / count), the numpy restatement of the rule
            (tests/smooth_ref.py, whole arrays at once), upload of the result; host clock up to a synchronise, the median of --reps; its result is compared with
            the device's on its bits.
  tick      SortTracker.update -> TrackedLifter.push as tools/tracked_bench.py times it, with and without a 2-D filter in front of the lift and a 3-D one behind
            it: host clock per tick up to a synchronise, median and 99th percentile.
Prints one JSON line per measurement.  None of the numbers is a pass / fail bar.
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
LIMITS = {"launches": 180, "host": 300, "tick": 480}               # seconds per child
J, CN, SLOTS, T, W_PX, H_PX = 17, 2, 32, 27, 1280, 720


def _events(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _rows(np, n, seed):
    g = np.random.default_rng(seed)
    return np.concatenate((g.uniform(0, 1000, (n, J, 2)), g.uniform(0, 1, (n, J, 1))), -1).astype(np.float32)


def _track_arrays(np, streams, count):
    """Every stream emits `count` tracks: ids 1 .. count on slots 0 .. count - 1, none just born."""
    ids, slot = np.full((streams, SLOTS), -1, np.int32), np.zeros((streams, SLOTS), np.int32)
    ids[:, :count], slot[:, :count] = np.arange(1, count + 1), np.arange(count)
    return dict(ids=ids, slot=slot, born=np.zeros((streams, SLOTS), np.int32), count=np.full(streams, count, np.int32))


def _shapes(np, rows):
    """(streams, rows mode, R, TrackResult arrays) of the tracked entry at 22 rows (one stream of 22 persons) and 1,024 rows (32 streams of 32 tracks)."""
    return (1, "persons", 22, _track_arrays(np, 1, 22)) if rows == 22 else (32, "tracks", 32, _track_arrays(np, 32, 32))


def step_launches(args):
    import numpy as np
    import torch
    from types import SimpleNamespace
    import kasportsformer_amd as K
    for rows in (22, 1024):
        x = torch.from_numpy(_rows(np, rows, rows)).cuda()
        f = K.OneEuroFilter(slots=rows)
        f.push(x)
        ms = statistics.median(_events(torch, lambda: f.push(x), args.iters) for _ in range(args.reps))
        print(json.dumps({"what": "OneEuroFilter.push (kasf_one_euro_push), per call", "rows": rows, "event_ms": round(ms, 5)}), flush=True)
        streams, mode, R, arrays = _shapes(np, rows)
        t = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in arrays.items()})
        ft = K.OneEuroFilter(streams=streams, track_slots=SLOTS, rows=mode, num_person=R)
        ft.push(x, t)
        ms = statistics.median(_events(torch, lambda: ft.push(x, t), args.iters) for _ in range(args.reps))
        print(json.dumps({"what": "OneEuroFilter.push(kp, TrackResult) (kasf_one_euro_tracked), per call", "rows": rows, "streams": streams,
                          "event_ms": round(ms, 5)}), flush=True)
    x = torch.from_numpy(_rows(np, 18000, 1)).cuda()
    K.smooth_tracks(x)
    ms = statistics.median(_events(torch, lambda: K.smooth_tracks(x), 3) for _ in range(args.reps))
    print(json.dumps({"what": "smooth_tracks (kasf_one_euro_tracks), one track", "frames": 18000, "event_ms": round(ms, 4),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


def step_host(args):
    import numpy as np
    import torch
    from types import SimpleNamespace
    import kasportsformer_amd as K
    from tests.smooth_ref import new_state, params, push_rows_np, tracks_np
    from tests.tracked_ref import tracked_front_np
    p, ticks = params(), 12

    def bits(a):
        return (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)
    for rows in (22, 1024):
        xs = [torch.from_numpy(_rows(np, rows, 100 * rows + i)).cuda() for i in range(ticks)]
        streams, mode, R, arrays = _shapes(np, rows)
        t = SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in arrays.items()})
        f, ft = K.OneEuroFilter(slots=rows), K.OneEuroFilter(streams=streams, track_slots=SLOTS, rows=mode, num_person=R)
        st, stt = new_state(rows, J, CN), new_state(streams * SLOTS, J, CN)

        def host_push(tick):
            return torch.from_numpy(push_rows_np(st, p, xs[tick].cpu().numpy(), None, tick, True)).cuda()

        def host_tracked(tick):
            got = {k: getattr(t, k).cpu().numpy() for k in ("ids", "slot", "born", "count")}
            x = xs[tick].cpu().numpy()
            row_slot, reset, _ = tracked_front_np(stt, got, mode, R)
            stt["last"][row_slot[reset & (row_slot >= 0)]] = -1
            ok = row_slot >= 0
            out = x.copy()
            out[ok] = push_rows_np(stt, p, x[ok], row_slot[ok], tick, True)
            return torch.from_numpy(out).cuda()
        for name, dev_fn, host_fn in (("push", lambda i: f.push(xs[i]), host_push), ("tracked", lambda i: ft.push(xs[i], t), host_tracked)):
            equal, dev_ms, host_ms = True, [], []
            for tick in range(ticks):
                d, e_d = _wall(torch, lambda: dev_fn(tick))
                h, e_h = _wall(torch, lambda: host_fn(tick))
                equal = equal and bool(np.array_equal(bits(d), bits(h)))
                dev_ms.append(e_d)
                host_ms.append(e_h)
            print(json.dumps({"what": f"{name}: device call vs download + numpy restatement + upload, host clock per tick", "rows": rows,
                              "device_wall_ms": round(statistics.median(dev_ms[2:]), 4), "host_path_wall_ms": round(statistics.median(host_ms[2:]), 4),
                              "bits_equal": equal}), flush=True)
    x = torch.from_numpy(_rows(np, 18000, 1)).cuda()
    K.smooth_tracks(x)
    d, e_d = _wall(torch, lambda: K.smooth_tracks(x))
    h, e_h = _wall(torch, lambda: torch.from_numpy(tracks_np(p, x.cpu().numpy(), [0, 18000], True)).cuda())
    print(json.dumps({"what": "one recorded track: smooth_tracks vs download + numpy restatement + upload, host clock", "frames": 18000,
                      "device_wall_ms": round(e_d, 4), "host_path_wall_ms": round(e_h, 2), "bits_equal": bool(np.array_equal(bits(d), bits(h)))}), flush=True)


def step_tick(args):
    import numpy as np
    import torch
    import kasportsformer_amd as K
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from tracked_bench import _boxes
    n = args.warmup + args.ticks
    for P in args.persons:
        g = np.random.default_rng(0)
        boxes = torch.from_numpy(_boxes(g, n, P)).cuda()
        count = torch.full((1,), P, dtype=torch.int32, device="cuda")
        kps = torch.from_numpy(np.concatenate((g.uniform((0, 0), (W_PX, H_PX), size=(n, P, 17, 2)), g.uniform(0, 1, size=(n, P, 17, 1))), -1).astype(np.float32)).cuda()
        model = K.KASportsFormer(n_layers=args.layers, num_heads=8, n_frames=T, compute_dtype=args.dtype).cuda().eval()
        kw = dict(streams=1, track_slots=SLOTS, rows="persons", num_person=P)
        trk = [K.SortTracker(streams=1, slots=SLOTS, min_hits=0, num_person=P, hold_last=True) for _ in range(2)]
        lift = [K.TrackedLifter(model, W_PX, H_PX, flip=True, lag=0, **kw) for _ in range(2)]
        f2, f3 = K.OneEuroFilter(**kw), K.OneEuroFilter(channels=3, score=False, **kw)

        def plain(i):
            return lift[0].push(kps[i], trk[0].update(boxes[i], count)).poses

        def filtered(i):
            t = trk[1].update(boxes[i], count)
            return f3.push(lift[1].push(f2.push(kps[i], t), t).poses, t)
        wall = {"plain": [], "filtered": []}
        for i in range(n):
            for name, fn in (("plain", plain), ("filtered", filtered)):
                _, ms = _wall(torch, lambda: fn(i))
                if i >= args.warmup:
                    wall[name].append(ms)
        stats = {k: {"median": round(statistics.median(v), 4), "p99": round(sorted(v)[min(len(v) - 1, int(0.99 * len(v)))], 4)} for k, v in wall.items()}
        print(json.dumps({"what": "SortTracker.update -> TrackedLifter.push per tick, without and with OneEuroFilter in front of and behind the lift (host clock)",
                          "persons": P, "layers": args.layers, "dtype": args.dtype, "ticks": args.ticks, "wall_ms": stats,
                          "added_ms_median": round(stats["filtered"]["median"] - stats["plain"]["median"], 4)}), flush=True)


STEPS = {"launches": step_launches, "host": step_host, "tick": step_tick}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs="+", choices=list(STEPS), default=list(STEPS))
    ap.add_argument("--child", choices=list(STEPS), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--persons", type=int, nargs="+", default=[2, 22])
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16")
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if any(not 1 <= P <= SLOTS for P in args.persons):
        ap.error(f"--persons must be in [1, {SLOTS}]")
    if args.child is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("smooth_bench: needs a GPU; there is no CPU path to time")
        STEPS[args.child](args)
        return
    passed = [a for a in sys.argv[1:]]
    for step in args.steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step] + passed, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            sys.exit(f"smooth_bench: step {step} did not finish in {LIMITS[step]} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"smooth_bench: step {step} ended with status {r.returncode}; nothing further is started")


if __name__ == "__main__":
    main()
