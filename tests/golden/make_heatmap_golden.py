#!/usr/bin/env python3
"""Generate the fixture of the heatmap decode from the REAL reference helpers (run in the build container only).

    python tests/golden/make_heatmap_golden.py       # needs the reference checkout (make_lift_golden.REF)

Imports ``demo/lib/hrnet/lib/utils/inference.py`` for ``get_final_preds`` / ``get_max_preds`` and ``demo/lib/hrnet/lib/utils/utilitys.py`` for
``box_to_center_scale`` and calls them as they are.  Two modules they import are not installed here and are shimmed IN THIS PROCESS ONLY:

  cv2          one function, ``getAffineTransform``: the 6 x 6 system OpenCV sets up for the three point pairs, solved with ``np.linalg.solve`` in float64.
               THE SOLVER IS THIS SHIM'S, not OpenCV's LU: the affine's six numbers carry this solver's ~1e-13 relative error, which is what moves a few
               image-space coordinates by one fp32 ulp against the closed form (neq_count below).
  torchvision  imported by utilitys.py for its PreProcess, which is not used: an empty module.

The refined heatmap-space coordinates are internal to ``get_final_preds``; they are recorded by wrapping the ``transform_preds`` name it calls (the wrapper
copies the ``coords`` argument and calls the reference's function).  Writes tensors only:

  heatmap_decode.npz, per group g (a: P = 5 persons of 96 x 72 maps in a 854 x 480 frame; b: 5 persons of 64 x 48 maps in a 8000 x 4320 frame)
    g_hm [P, 17, H, W]          float16 (every value is fp16-representable, so fp32 / fp16 tests share them): Gaussian blobs, some against the border, on an
                                exactly-zero background with sparse noise; the last person is hand-made (edge_person)
    g_center, g_scale [P, 2]    float32: where the crop sits, independent of the boxes
    g_boxes [P, 4], g_aspect    float32 x1, y1, x2, y2 (one with center x == -1) and the float64 frame_height / frame_width the demo passes (utilitys.py:151)
    g_box_center, g_box_scale   box_to_center_scale(box as float64, frame_height, frame_width)
    g_maxpos [P, 17, 2], g_maxvals [P, 17, 1]        get_max_preds
    g_coords_r{0,1} [P, 17, 2]  the coords transform_preds was given, POST_PROCESS off / on
    g_preds_cs_r{0,1}           get_final_preds with g_center / g_scale
    g_preds_box_r{0,1}          get_final_preds with g_box_center / g_box_scale
  neq_count, max_ulp            tests/test_heatmap_cpu.py's heatmap_decode_np against all eight preds arrays: how many coordinates are not bit-equal, and the
                                largest distance in fp32 ulps
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from make_lift_golden import REF  # noqa: E402

F32 = np.float32


def shim_missing_modules():
    def get_affine_transform(src, dst):
        src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
        a, b = np.zeros((6, 6)), np.zeros(6)
        for i in range(3):
            a[2 * i, 0:2], a[2 * i, 2] = src[i], 1.0
            a[2 * i + 1, 3:5], a[2 * i + 1, 5] = src[i], 1.0
            b[2 * i], b[2 * i + 1] = dst[i]
        return np.linalg.solve(a, b).reshape(2, 3)

    for name in ("cv2", "torchvision", "torchvision.transforms"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            print("shimmed", name)
    if not hasattr(sys.modules["cv2"], "getAffineTransform"):
        sys.modules["cv2"].getAffineTransform = get_affine_transform
    if "transforms" not in vars(sys.modules["torchvision"]):
        sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]


def put(m, y, x, peak, left=0.0, right=0.0, up=0.0, down=0.0):
    """A maximum at (y, x) with the given four neighbours, where they exist."""
    H, W = m.shape
    m[y, x] = peak
    for (yy, xx), v in (((y, x - 1), left), ((y, x + 1), right), ((y - 1, x), up), ((y + 1, x), down)):
        if 0 <= yy < H and 0 <= xx < W:
            m[yy, xx] = v


def edge_person(H, W):
    """17 hand-made maps (tests/test_heatmap_cpu.py reads this order)."""
    p = np.zeros((17, H, W), F32)
    for (y, x) in ((7, 20), (H - 10, W - 5)):                  # 0: two equal maxima far apart: the first in row-major order counts
        put(p[0], y, x, 0.75, left=0.25, right=0.5, up=0.5, down=0.25)
    #                                                            1: all zero: "maxval > 0" is false, (0, 0)
    p[2] = -0.5                                                # 2: all negative, the maximum inside: (0, 0) all the same
    p[2, H // 2, W // 2] = -0.25
    for j, x in zip((3, 4, 5, 6), (0, 1, W - 2, W - 1)):       # 3-6: x against the strict bounds 1 < x < W - 1: only W - 2 is refined
        put(p[j], H // 2, x, 1.0, left=0.25, right=0.5, up=0.125, down=0.5)
    for j, y in zip((7, 8, 9, 10), (0, 1, H - 2, H - 1)):      # 7-10: the same in y
        put(p[j], y, W // 2, 1.0, left=0.25, right=0.5, up=0.125, down=0.5)
    put(p[11], 30, 40, 0.875, left=0.5, right=0.5, up=0.25, down=0.125)      # 11: equal neighbours in x: sign(0) = 0
    put(p[12], 31, 41, 0.875, left=0.125, right=0.25, up=0.5, down=0.5)      # 12: equal neighbours in y
    put(p[13], 12, 13, 0.625, left=0.5, right=0.25, up=0.5, down=0.25)       # 13: both steps negative
    for (y, x) in ((H - 3, 5), (20, W - 9), (20, 9)):          # 14: three equal maxima; row-major first is (20, 9)
        put(p[14], y, x, 0.5, left=0.125, right=0.25, up=0.125, down=0.25)
    put(p[15], 2, 2, 1.0, left=0.25, right=0.5, up=0.5, down=0.25)           # 15: the first refined column and row
    put(p[16], H - 3, W - 3, 1.0, left=0.5, right=0.25, up=0.25, down=0.5)   # 16: well inside, steps of opposite signs
    return p


def blob_persons(g, P, H, W):
    """Gaussian blobs (sigma 1.5-3, amplitude 0.3-1, centers up to 2 px outside the map) on an exactly-zero background, plus noise in 1 % of the pixels."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    hm = np.zeros((P, 17, H, W), np.float64)
    for p in range(P):
        for j in range(17):
            cy, cx = g.uniform(-2, H + 1), g.uniform(-2, W + 1)
            s, amp = g.uniform(1.5, 3.0), g.uniform(0.3, 1.0)
            blob = amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            blob[blob < 0.01] = 0.0
            noise = np.where(g.uniform(size=(H, W)) < 0.01, g.uniform(-0.05, 0.05, size=(H, W)), 0.0)
            hm[p, j] = blob + noise
    return hm.astype(np.float16)


def geometry(g, P, fw, fh):
    center = np.stack((g.uniform(0, fw, P), g.uniform(0, fh, P)), axis=-1).astype(F32)
    scale = (g.uniform(0.3, fh / 200.0, size=(P, 1)) * np.array([0.75, 1.0])).astype(F32)
    x1, y1 = g.uniform(0, fw * 0.7, P), g.uniform(0, fh * 0.5, P)
    bw, bh = g.uniform(0.05, 0.3, P) * fw, g.uniform(0.2, 0.5, P) * fh
    bw[1] = bh[1] * 4                                          # one box wider than the aspect, the others taller
    boxes = np.stack((x1, y1, x1 + bw, y1 + bh), axis=-1).astype(F32)
    boxes[2, 0], boxes[2, 2] = -3.0, 1.0                       # center x == -1: no 1.25 (utilitys.py:132)
    return center, scale, boxes


def main():
    shim_missing_modules()
    sys.path.insert(0, os.path.join(REF, "demo"))
    from lib.hrnet.lib.utils import inference
    from lib.hrnet.lib.utils.utilitys import box_to_center_scale
    from test_heatmap_cpu import heatmap_decode_np, ulp_distance

    seen = []
    reference_transform = inference.transform_preds

    def recording_transform(coords, center, scale, output_size):
        seen.append(np.array(coords, copy=True))
        return reference_transform(coords, center, scale, output_size)

    inference.transform_preds = recording_transform
    g = np.random.default_rng(2025)
    out, neq, worst = {}, 0, 0
    for name, (H, W), (fw, fh) in (("a", (96, 72), (854, 480)), ("b", (64, 48), (8000, 4320))):
        hm16 = np.concatenate((blob_persons(g, 4, H, W), edge_person(H, W).astype(np.float16)[None]))
        hm = hm16.astype(F32)
        assert np.array_equal(hm.astype(np.float16), hm16)
        P = hm.shape[0]
        center, scale, boxes = geometry(g, P, fw, fh)
        aspect = np.float64(fh) / np.float64(fw)
        derived = [box_to_center_scale(b.astype(np.float64), fh, fw) for b in boxes]       # (model_image_width, model_image_height) = shape[0], shape[1]
        box_center, box_scale = np.stack([d[0] for d in derived]), np.stack([d[1] for d in derived])
        assert box_center.dtype == box_scale.dtype == F32
        maxpos, maxvals = inference.get_max_preds(hm.copy())
        out.update({f"{name}_hm": hm16, f"{name}_center": center, f"{name}_scale": scale, f"{name}_boxes": boxes, f"{name}_aspect": aspect,
                    f"{name}_box_center": box_center, f"{name}_box_scale": box_scale, f"{name}_maxpos": maxpos, f"{name}_maxvals": maxvals})
        for r in (0, 1):
            cfg = types.SimpleNamespace(TEST=types.SimpleNamespace(POST_PROCESS=bool(r)))
            for tag, c, s, kw in (("cs", center, scale, dict(center=center, scale=scale)), ("box", box_center, box_scale, dict(boxes=boxes, aspect=aspect))):
                del seen[:]
                keep = hm.copy()
                preds, mv = inference.get_final_preds(cfg, hm, c, s)
                assert np.array_equal(hm, keep) and np.array_equal(mv, maxvals) and preds.dtype == F32 and len(seen) == P
                out[f"{name}_preds_{tag}_r{r}"] = preds
                out[f"{name}_coords_r{r}"] = np.stack(seen)
                d = ulp_distance(heatmap_decode_np(hm16, refine=bool(r), **kw)[..., :2], preds)
                neq, worst = neq + int((d != 0).sum()), max(worst, int(d.max()))
    out["neq_count"], out["max_ulp"] = np.array(neq, np.int64), np.array(worst, np.int64)
    path = os.path.join(HERE, "heatmap_decode.npz")
    np.savez_compressed(path, **out)
    print("wrote heatmap_decode.npz:", {k: v.shape for k, v in out.items()}, "neq_count", neq, "max_ulp", worst, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
