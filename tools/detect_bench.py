#!/usr/bin/env python3
"""YOLOv3 detector output in, person boxes out: the decode on the device against the host path it replaces.

    python tools/detect_bench.py [--reps 7] [--kernel-iters 50] [--persons 12] [--seed 0]

A 416 x 416 network (heads of 13, 26 and 52 cells, 3 anchors, 80 classes: N = 10,647 candidates per image), frames of 1280 x 720, confidence 0.30, nms 0.4.
Every image has background objectness logits around -6 and --persons planted persons, each with two duplicates in neighbouring cells and a third of them
doubled by another object class.
  decode   kasf_detect_boxes alone (its two launches: selection, then sort + NMS + output) at B = 1 and B = 64, raw fp16 heads and the fp32 prediction:
           CUDA events around --kernel-iters back-to-back calls, per call, median and minimum of --reps, with the bytes the selection has to read at least
           (heads form: the objectness planes; prediction form: one 64-byte sector per row) and the size of the whole input.
  host     the path it replaces, for the same fp32 prediction: the device-to-host copy (write_results' nonzero() / squeeze() calls synchronise for every kept
           box; one copy is the cheapest host route) plus tests/test_detect_cpu.py's numpy restatement, host clock, median of --reps; the boxes of both ways
           are compared on their bits.  And the device call as a caller sees it (Python surface, host clock up to a synchronise).
Prints one JSON line.
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
from kasportsformer_amd._args import stream  # noqa: E402
from tests.test_detect_cpu import detect_decode_np  # noqa: E402

INP, GRIDS, A, NC, W_PX, H_PX, CONF, NMS = 416, (13, 26, 52), 3, 80, 1280, 720, 0.30, 0.4


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def _heads(seed, B, persons):
    """Three fp16 heads [B,255,G,G] on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    heads = []
    for G in GRIDS:
        t = torch.randn((B, A, 5 + NC, G, G), device="cuda", generator=g)
        t[:, :, 2:4] *= 0.4
        t[:, :, 4] = t[:, :, 4] * 0.7 - 6.0
        t[:, :, 5:] -= 4.0
        heads.append(t)
    for b in range(B):
        for n in range(persons):
            k = int(rng.integers(0, 3))
            G = GRIDS[k]
            a, cy, cx = int(rng.integers(0, A)), int(rng.integers(1, G - 1)), int(rng.integers(1, G - 1))
            size = np.log(rng.uniform(0.1, 0.3, 2) * INP / np.array(K.YOLOV3_ANCHORS[K.YOLOV3_MASKS[k][a]]))
            for dy, dx in ((0, 0), (0, 1), (1, 0)):
                t = heads[k]
                t[b, a, 0:2, cy + dy, cx + dx] = torch.tensor([2.0 - 4.0 * dx, 2.0 - 4.0 * dy], device="cuda")
                t[b, a, 2:4, cy + dy, cx + dx] = torch.tensor(size + rng.normal(size=2) * 0.05, dtype=torch.float32, device="cuda")
                t[b, a, 4, cy + dy, cx + dx] = float(rng.uniform(-0.5, 4.0))
                t[b, a, 5:, cy + dy, cx + dx] = -4.0
                t[b, a, 5 + (0 if n % 3 or (dy, dx) == (0, 0) else 17), cy + dy, cx + dx] = 4.0
    return [t.reshape(B, A * (5 + NC), t.shape[3], t.shape[4]).half().contiguous() for t in heads]


def _prediction(heads):
    """predict_transform of the heads in torch on the device: [B,N,85] fp32, what the detector network's forward returns."""
    out = []
    for hd, mask in zip(heads, K.YOLOV3_MASKS):
        B, _, G, _ = hd.shape
        stride = INP // G
        t = hd.float().view(B, A, 5 + NC, G * G).permute(0, 3, 1, 2).contiguous()
        cell = torch.arange(G * G, device="cuda")
        anc = torch.tensor([[K.YOLOV3_ANCHORS[i][0] / stride, K.YOLOV3_ANCHORS[i][1] / stride] for i in mask], device="cuda")
        t[..., 0] = (torch.sigmoid(t[..., 0]) + (cell % G).view(1, -1, 1)) * stride
        t[..., 1] = (torch.sigmoid(t[..., 1]) + (cell // G).view(1, -1, 1)) * stride
        t[..., 2:4] = torch.exp(t[..., 2:4]) * anc * stride
        t[..., 4:] = torch.sigmoid(t[..., 4:])
        out.append(t.view(B, G * G * A, 5 + NC))
    return torch.cat(out, dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--persons", type=int, default=12)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    lib = _lib.load()
    N = sum(g * g * A for g in GRIDS)
    res = {"what": "detector output in, person boxes out (measured; CUDA events for the device, host clock for the host path, median of %d)" % args.reps,
           "inp_dim": INP, "candidates_per_image": N, "classes": NC, "device": torch.cuda.get_device_name(0)}
    decode, host = {}, {}
    anchors = np.array([K.YOLOV3_ANCHORS[i] for m in K.YOLOV3_MASKS for i in m], np.float32).reshape(-1)
    for B in (1, 64):
        heads = _heads(args.seed + B, B, args.persons)
        pred = _prediction(heads)
        wh = torch.tensor([[W_PX, H_PX]] * B, dtype=torch.float32, device="cuda")
        boxes, index = torch.empty((B, 32, 6), device="cuda"), torch.empty((B, 32), dtype=torch.int32, device="cuda")
        count = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        nbytes = lib.kasf_detect_workspace_bytes(B, N, 1024)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        forms = (("fp16 heads", _lib.DETECT_HEADS, _lib.DTYPE_F16, heads, list(GRIDS), B * N * 2, sum(h.numel() for h in heads) * 2),
                 ("fp32 prediction", _lib.DETECT_PREDICTION, _lib.DTYPE_F32, [pred], [N], B * N * 64, pred.numel() * 4))
        for name, form, code, tensors, grids, least, whole in forms:
            ptrs = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
            grid = (C.c_int32 * len(grids))(*grids)

            def launch():
                return lib.kasf_detect_boxes(ptrs, len(tensors), form, code, B, grid, A, NC, anchors.ctypes.data_as(C.POINTER(C.c_float)), INP, wh.data_ptr(),
                                             CONF, NMS, 0, 1024, 32, boxes.data_ptr(), index.data_ptr(), count.data_ptr(), ws.data_ptr(), nbytes, stream())
            for _ in range(3):
                _lib.check(launch())
            reps = []
            for _ in range(args.reps):
                _, e, _ = _timed(lambda: [_lib.check(launch()) for _ in range(args.kernel_iters)])
                reps.append(e / args.kernel_iters)
            c = count.cpu().numpy()
            decode[f"{name} @ B={B}"] = {"us": round(statistics.median(reps) * 1e3, 2), "min_us": round(min(reps) * 1e3, 2), "input_MB": round(whole / 1e6, 2),
                                         "least_read_MB": round(least / 1e6, 3), "workspace_MB": round(nbytes / 1e6, 2),
                                         "boxes_per_image": round(float(c[:, 0].mean()), 1), "candidates_per_image": round(float(c[:, 1].mean()), 1)}
        # the host path: D2H copy + numpy, from the same device tensor
        want = K.detections_to_boxes(pred, W_PX, H_PX, INP, confidence=CONF, nms=NMS)
        copy_ms, numpy_ms, total_ms = [], [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            on_host = pred.cpu().numpy()
            t1 = time.perf_counter()
            got = detect_decode_np(on_host, W_PX, H_PX, INP, confidence=CONF, nms=NMS)
            t2 = time.perf_counter()
            copy_ms.append((t1 - t0) * 1e3)
            numpy_ms.append((t2 - t1) * 1e3)
            total_ms.append((t2 - t0) * 1e3)
        equal = bool(torch.equal(torch.from_numpy(got[0]), want.boxes.cpu()) and torch.equal(torch.from_numpy(got[3]), want.index.cpu()))
        host[f"fp32 prediction @ B={B}"] = {"d2h_copy_ms": round(statistics.median(copy_ms), 4), "numpy_decode_ms": round(statistics.median(numpy_ms), 4),
                                            "total_ms": round(statistics.median(total_ms), 4), "equal_to_device": equal}
        call = lambda: K.detections_to_boxes(pred, W_PX, H_PX, INP, confidence=CONF, nms=NMS)
        call()
        host[f"fp32 prediction @ B={B}"]["device_call_wall_ms"] = round(statistics.median([_timed(call)[2] for _ in range(args.reps)]), 4)
        call = lambda: K.yolo_heads_to_boxes(heads, W_PX, H_PX, INP, confidence=CONF, nms=NMS)
        call()
        host[f"fp32 prediction @ B={B}"]["device_call_wall_ms_fp16_heads"] = round(statistics.median([_timed(call)[2] for _ in range(args.reps)]), 4)
        del heads, pred
    res["decode_entry"], res["host_path"] = decode, host
    print(json.dumps(res))


if __name__ == "__main__":
    main()
