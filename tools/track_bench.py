#!/usr/bin/env python3
"""Person boxes in, tracked person boxes out: SortTracker.update alone on the device, and the host path it replaces for the same inputs.

    python tools/track_bench.py [--ticks 200] [--warmup 20] [--seed 0] [--out FILE.json]

Seeded synthetic players in a 1280 x 720 frame (tests/test_track_cpu.py, ``players``): 1 and 22 tracked persons with slots = 32 and 32 detection rows, and 64
persons with slots = 64 and 64 rows (every lane of the wavefront taken, a 64 x 64 assignment every tick), each at B = 1 and B = 16 streams (the same
sequence with its own seed per stream).  The detections and counts of every tick sit on the device before the clock starts, as ``detections_to_boxes``
leaves them.
  device   ``trk.update(boxes, count)`` per tick after --warmup ticks: CUDA events around the one call (median and 99th percentile over --ticks ticks), and in
           a second pass over the same ticks the host clock around the call plus a synchronise.
  host     the path the call replaces: device-to-host copy of boxes and count (which waits for the device), ``sort_update_np`` per stream -- the numpy / scipy
           restatement of tests/test_track_cpu.py; the reference's numba, filterpy and scipy path is not installed here, so this is NOT ``Sort.update`` itself --
           and the upload of the tracked boxes; host clock, median and 99th percentile; labelled "numpy / scipy restatement".  The ids of both ways are compared.
Prints one JSON line; --out also writes it to a file (stamp it with tools/stamp.py --embed).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kasportsformer_amd as K  # noqa: E402
from tests.test_track_cpu import new_tracker, pad, players, sort_update_np  # noqa: E402

CONFIGS = (("1 person", 1, dict(slots=32), 32, dict()),
           ("22 persons", 22, dict(slots=32), 32, dict(grid=(6, 4), box=((30, 50), (60, 100)), speed=0.5, p_miss=0.02, p_fp=0.02)),
           ("64 x 64 full", 64, dict(slots=64), 64, dict(grid=(8, 8), box=((30, 50), (40, 60)), speed=0.3, p_miss=0.0, p_fp=0.0)))


def stats(ms):
    v = np.sort(np.asarray(ms, np.float64))
    return {"median_us": round(float(np.median(v)) * 1e3, 2), "p99_us": round(float(v[min(len(v) - 1, int(np.ceil(0.99 * len(v))) - 1)]) * 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench.py needs a GPU: a timing taken without one says nothing")
    T, W = args.ticks, args.warmup
    res = {"what": "person boxes in, tracked person boxes out, per tick (measured; CUDA events and host clock, median and 99th percentile of %d ticks)" % T,
           "device": torch.cuda.get_device_name(0), "rows": {}}
    params = dict(min_hits=0, max_age=1)
    for label, people, size, rows, kw in CONFIGS:
        for B in (1, 16):
            padded = [pad(players(args.seed + 100 * b + people, people, ticks=T + W, **kw), rows) for b in range(B)]
            dets = np.ascontiguousarray(np.stack([p[0] for p in padded], axis=1))          # [ticks, B, rows, 5]
            count = np.ascontiguousarray(np.stack([p[1] for p in padded], axis=1))
            d, c = torch.from_numpy(dets).cuda(), torch.from_numpy(count).cuda()
            # device: events
            trk = K.SortTracker(streams=B, **size, **params)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(T)]
            ids_dev = []
            for t in range(W + T):
                if t >= W:
                    ev[t - W][0].record()
                r = trk.update(d[t], c[t])
                if t >= W:
                    ev[t - W][1].record()
                ids_dev.append((r.ids, r.count))
            torch.cuda.synchronize()
            event_ms = [a.elapsed_time(b) for a, b in ev]
            ids_dev = [(i.cpu().numpy(), n.cpu().numpy()) for i, n in ids_dev]
            # device: host clock around call + synchronise
            trk.reset()
            wall_ms = []
            for t in range(W + T):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                trk.update(d[t], c[t])
                torch.cuda.synchronize()
                if t >= W:
                    wall_ms.append((time.perf_counter() - t0) * 1e3)
            # host: copy down, restatement, upload
            hosts = [new_tracker(**size, **params) for _ in range(B)]
            host_ms, same = [], True
            for t in range(W + T):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bx, cn = d[t].cpu().numpy(), c[t].cpu().numpy()
                out = np.zeros((B, size["slots"], 4), np.float32)
                for b in range(B):
                    rr = sort_update_np(hosts[b], bx[b], cn[b])
                    out[b, :rr["count"]] = rr["boxes"]
                    same = same and rr["count"] == ids_dev[t][1][b] and np.array_equal(rr["ids"], ids_dev[t][0][b, :rr["count"]])
                up = torch.from_numpy(out).cuda()
                torch.cuda.synchronize()
                if t >= W:
                    host_ms.append((time.perf_counter() - t0) * 1e3)
            del up
            res["rows"][f"{label}, B = {B}"] = {"device_events": stats(event_ms), "device_host_clock": stats(wall_ms),
                                                "host_path (numpy / scipy restatement, NOT Sort.update itself)": stats(host_ms), "ids_equal": bool(same)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
