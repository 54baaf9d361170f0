#!/usr/bin/env python3
"""Generate the fixture of the detector decode from the REAL reference helpers (run in the build container only).

    python tests/golden/make_detect_golden.py       # needs the reference checkout (make_lift_golden.REF)

Imports ``demo/lib/yolov3/util.py`` and calls its ``predict_transform`` (once per head, on fp32 copies of the fp16 heads, CUDA = False) and its
``write_results(prediction, 0.30, 80, nms=True, nms_conf=0.4, det_hm=True)`` as they are, ONE IMAGE PER CALL: ``write_results`` returns at the first image
without a person, which would hide the later ones.  ``cv2`` is not installed here; util.py and bbox.py import it and these functions do not use it, so it is
shimmed as an empty module IN THIS PROCESS ONLY.  The un-letterbox is ``yolo_human_det``'s own lines (demo/lib/yolov3/human_detector.py:144-153): that
function needs the network, so the ten lines are read from the reference file when this script runs and executed on the result, as they are; no reference text
is kept here.  Writes arrays only:

  detect_decode.npz, per group g (a: inp_dim 96, grids 3 / 6 / 12, N = 567, frame 854 x 480; b: inp_dim 160, grids 5 / 10 / 20, N = 1,575, frame 1080 x 1920)
    g_head0, g_head1, g_head2 [3, 255, G, G]   float16 raw heads, stride 32 first.  A few background values (the file has to stay small), and per image 5
                                planted persons with 2-3 overlapping duplicates each (a neighbouring cell, another anchor, another head), 2 planted
                                non-person objects, and persons reaching outside the frame
    g_inp_dim, g_frame          int32, float32 (width, height)
    g_prediction [3, N, 85]     float32: the reference's predict_transform of the three heads, concatenated as Darknet.forward does
    g_ref_boxes [3, 32, 6], g_ref_count [3], g_ref_index [3, 32]   the reference's rows (x1, y1, x2, y2 in frame pixels, objectness, class score), zero / -1
                                padded; the candidate index of a row is recovered by matching its objectness in g_prediction
    g_candidates [3]            person candidates above the threshold, counted on g_prediction
    g_f64_boxes (float64), g_f64_count, g_f64_index                 rules 2-8 evaluated in float64 from the heads (tests/test_detect_cpu.py, ft = float64)
    g_ref_err_xy, g_ref_err_score   the largest |reference - float64| over the coordinates and over the two scores

Asserted, and re-drawn with the next seed until they hold (the margins that make the survivor sets independent of the last bit of any exp):
  every candidate's |objectness - confidence| >= 1e-3; objectness gaps between candidates >= 1e-4; |iou - nms| >= 1e-3 for every pair NMS compares;
  person-vs-best-other class logit margin >= 0.05 on every candidate above the threshold; at least 5 survivors and 2 suppressed candidates per image.
"""
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_lift_golden import REF  # noqa: E402
from test_detect_cpu import ANCHORS, MASKS, detect_decode_np, heads_to_prediction_np  # noqa: E402

F32, F64 = np.float32, np.float64
C, A, B, CONF, NMS = 80, 3, 3, 0.30, 0.4
GROUPS = {"a": (96, 854, 480), "b": (160, 1080, 1920)}


def reference():
    try:
        import cv2  # noqa: F401
    except ImportError:
        sys.modules["cv2"] = types.ModuleType("cv2")
        print("shimmed cv2")
    sys.path.insert(0, os.path.join(REF, "demo"))
    from lib.yolov3 import util
    lines = open(os.path.join(REF, "demo", "lib", "yolov3", "human_detector.py")).read().splitlines()[143:153]
    text = textwrap.dedent("\n".join(lines))
    assert text.startswith("img_dim = ") and "scaling_factor" in text and "clamp" in lines[-1], "human_detector.py:144-153 moved"
    return util, compile(text, "human_detector.py:144-153", "exec")


def logit(p):
    return np.log(p / (1.0 - p))


def draw(rng, inp, fw, fh):
    """Three fp16 heads [B, 255, G, G] for one group."""
    grids = [inp // 32, inp // 16, inp // 8]
    heads = []
    for G in grids:
        t = np.empty((B, A, 5 + C, G, G), F64)
        pick = lambda vals, p: rng.choice(vals, size=(B, A, G, G), p=p)
        for i in range(4):
            t[:, :, i] = pick([0.0, 0.5, -0.5, 0.25], [0.85, 0.05, 0.05, 0.05])
        t[:, :, 4] = pick([-6.0, -5.5, -6.5, -7.0], [0.9, 0.04, 0.03, 0.03])
        for i in range(C):
            t[:, :, 5 + i] = pick([-4.0, -3.0, -5.0, -2.5], [0.92, 0.03, 0.03, 0.02])
        heads.append(t)
    sf = min(inp / fw, inp / fh)
    cw, ch = sf * fw, sf * fh                                                   # the letterboxed content
    ox, oy = (inp - cw) / 2, (inp - ch) / 2

    def plant(b, k, a, px, py, bw, bh, obj, cls):
        G, t = grids[k], heads[k]
        stride = inp // G
        cx, cy = min(max(int(px // stride), 0), G - 1), min(max(int(py // stride), 0), G - 1)
        fx, fy = min(max(px / stride - cx, 0.04), 0.96), min(max(py / stride - cy, 0.04), 0.96)
        aw, ah = ANCHORS[MASKS[k][a]]
        t[b, a, 0, cy, cx], t[b, a, 1, cy, cx] = logit(fx), logit(fy)
        t[b, a, 2, cy, cx], t[b, a, 3, cy, cx] = np.log(bw / aw), np.log(bh / ah)
        t[b, a, 4, cy, cx] = obj
        t[b, a, 5:, cy, cx] = -4.0
        t[b, a, 5 + cls, cy, cx] = 3.0
        t[b, a, 5 + (cls + 7) % C, cy, cx] = rng.choice([-1.0, 0.5, 2.0])      # a runner-up, well below the winner

    for b in range(B):
        objs = list(rng.permutation(np.arange(-0.3, 3.6, 0.06)))                # objectness logits: distinct, sigmoid gaps >= 1e-3
        used = set()

        def free(k, a, px, py):
            G = grids[k]
            stride = inp // G
            key = (k, a, min(max(int(py // stride), 0), G - 1), min(max(int(px // stride), 0), G - 1))
            if key in used:
                return False
            used.add(key)
            return True

        slots = [(0.04, 0.5), (0.3, 0.1), (0.55, 0.92), (0.8, 0.35), (0.97, 0.7)]
        for n, (u, v) in enumerate(slots):
            px, py = ox + (u + rng.uniform(-0.03, 0.03)) * cw, oy + (v + rng.uniform(-0.03, 0.03)) * ch
            bw, bh = rng.uniform(0.12, 0.2) * inp, rng.uniform(0.2, 0.34) * inp
            k, a = int(rng.integers(0, 3)), int(rng.integers(0, A))
            assert free(k, a, px, py)
            plant(b, k, a, px, py, bw, bh, objs.pop(), 0)
            stride = inp // grids[k]
            dups = [(k, a, px + stride * rng.choice([-1, 1]), py), ((k + 1) % 3, int(rng.integers(0, A)), px, py), (k, (a + 1) % A, px, py)]
            for dk, da, dx, dy in dups[:2 + n % 2]:
                if free(dk, da, dx, dy):
                    j = rng.uniform(-0.03, 0.03, 4) * inp * 0.3
                    plant(b, dk, da, dx + j[0], dy + j[1], bw + j[2], bh + j[3], objs.pop(), 0)
        for n in range(2):                                                      # not persons
            px, py = ox + rng.uniform(0.2, 0.8) * cw, oy + rng.uniform(0.2, 0.8) * ch
            k, a = int(rng.integers(0, 3)), int(rng.integers(0, A))
            if free(k, a, px, py):
                plant(b, k, a, px, py, 0.2 * inp, 0.2 * inp, objs.pop(), 17 + 20 * n)
    return [t.reshape(B, A * (5 + C), t.shape[3], t.shape[4]).astype(np.float16) for t in heads]


def run_reference(util, unletterbox, heads, inp, fw, fh):
    import torch
    preds = []
    for hd, mask in zip(heads, MASKS):
        t = torch.from_numpy(hd.astype(F32)).clone()
        preds.append(util.predict_transform(t, inp, [ANCHORS[i] for i in mask], C, False))
    prediction = torch.cat(preds, 1)
    assert prediction.dtype == torch.float32
    boxes, index, count = np.zeros((B, 32, 6), F32), np.full((B, 32), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        output = util.write_results(prediction[b:b + 1].clone(), CONF, C, nms=True, nms_conf=NMS, det_hm=True)
        assert output.dim() == 2 and output.shape[1] == 8 and (output[:, 0] == 0).all() and (output[:, 7] == 0).all()
        ns = {"torch": torch, "inp_dim": inp, "output": output, "img_dim": torch.FloatTensor((fw, fh)).repeat(1, 2)}   # img_dim as human_detector.py:131-132 leaves it
        exec(unletterbox, ns)
        out = ns["output"].numpy()
        n = len(out)
        assert n <= 32
        boxes[b, :n], count[b] = out[:, 1:7], n
        for r in range(n):
            hit = np.nonzero(prediction[b, :, 4].numpy() == out[r, 5])[0]
            assert len(hit) == 1
            index[b, r] = hit[0]
    return prediction.numpy(), boxes, index, count


def margins_hold(heads, prediction, inp, fw, fh):
    pred64, arg = heads_to_prediction_np(heads, inp, ft=F64)
    trace = []
    b64 = detect_decode_np(heads, fw, fh, inp, form="heads", confidence=CONF, nms=NMS, ft=F64, trace=trace)
    obj = pred64[..., 4]
    if np.abs(obj - F64(F32(CONF))).min() < 1e-3:
        return None
    if trace and np.abs(np.array([v for _, v in trace]) - F64(F32(NMS))).min() < 1e-3:
        return None
    for b in range(B):
        above = obj[b] > CONF
        person = above & (arg[b] == 0)
        o = np.sort(obj[b][person])
        if len(o) > 1 and np.diff(o).min() < 1e-4:
            return None
        logits = np.concatenate([h[b].astype(F64).reshape(A, 5 + C, -1).transpose(2, 0, 1).reshape(-1, 5 + C) for h in heads])[:, 5:]
        top2 = np.sort(logits[above], axis=1)[:, -2:]
        if (top2[:, 1] - top2[:, 0]).min() < 0.05:
            return None
        if b64[1][b] < 5 or b64[2][b] - b64[1][b] < 2:
            return None
    return b64


def main():
    util, unletterbox = reference()
    out = {}
    for g, (inp, fw, fh) in GROUPS.items():
        for seed in range(100):
            rng = np.random.default_rng(20261017 + 1000 * seed + ord(g))
            heads = draw(rng, inp, fw, fh)
            b64 = margins_hold(heads, None, inp, fw, fh)
            if b64 is not None:
                break
            print(f"group {g}: seed {seed} misses a margin, drawing again")
        else:
            raise SystemExit("no draw met the margins")
        prediction, boxes, index, count = run_reference(util, unletterbox, heads, inp, fw, fh)
        assert np.array_equal(count, b64[1]) and np.array_equal(index, b64[3]), "the reference and the fp64 evaluation keep the same candidates in the same order"
        n_mask = np.arange(32)[None, :, None] < count[:, None, None]
        err = np.abs(boxes.astype(F64) - b64[0]) * n_mask
        exy, esc = err[..., :4].max(), err[..., 4:].max()
        cands = ((prediction[..., 4] > F32(CONF)) & (np.argmax(prediction[..., 5:], axis=2) == 0)).sum(axis=1).astype(np.int32)
        assert np.array_equal(cands, b64[2])
        print(f"group {g}: seed {seed}, counts {count.tolist()} of {cands.tolist()} candidates, ref_err_xy {exy:.3e}, ref_err_score {esc:.3e}")
        for k in range(3):
            out[f"{g}_head{k}"] = heads[k]
        out.update({f"{g}_inp_dim": np.int32(inp), f"{g}_frame": np.array([fw, fh], F32), f"{g}_prediction": prediction, f"{g}_ref_boxes": boxes,
                    f"{g}_ref_count": count, f"{g}_ref_index": index, f"{g}_candidates": cands, f"{g}_f64_boxes": b64[0], f"{g}_f64_count": b64[1],
                    f"{g}_f64_index": b64[3], f"{g}_ref_err_xy": F64(exy), f"{g}_ref_err_score": F64(esc)})
    path = os.path.join(HERE, "detect_decode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
