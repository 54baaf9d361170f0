#!/usr/bin/env python3
"""Generate the fixture of the flip-tested heatmap decode from the REAL reference helpers (run in the build container only).

    python tests/golden/make_heatmap_flip_golden.py       # needs the reference checkout (make_lift_golden.REF)

Imports ``demo/lib/hrnet/lib/utils/transforms.py`` for ``flip_back`` and ``demo/lib/hrnet/lib/utils/inference.py`` for ``get_final_preds`` / ``get_max_preds``
through the in-process shims of make_heatmap_golden.py (``cv2.getAffineTransform`` is that file's float64 solve, not OpenCV's) and calls them as they are.
Between the two calls stand the two lines HRNet's evaluation applies when FLIP_TEST and SHIFT_HEATMAP are set (w48_384x288_adam_lr1e-3.yaml:119-121), in
float32 numpy:

    output_flipped[:, :, :, 1:] = output_flipped.copy()[:, :, :, 0:-1]
    output = (output + output_flipped) * 0.5

Writes tensors only:

  heatmap_flip.npz, per group g (a: P = 4 persons of 96 x 72 maps in a 854 x 480 frame; b: 4 persons of 64 x 48 maps in a 8000 x 4320 frame)
    g_hm, g_hmf [P, 17, H, W]   float16 (every value is fp16-representable): the network's output for the crops and for the mirrored crops.  Three persons of
                                Gaussian blobs whose mirrored partner lands within a pixel or two (one column to the left before the shift, as a real network's
                                does), sparse noise; the last person is hand-made (merge_person)
    g_center, g_scale [P, 2]    float32: where the crop sits
    g_merged [P, 17, H, W]      float32: (hm + shifted flip_back(hmf)) * 0.5
    g_maxpos [P, 17, 2], g_maxvals [P, 17, 1]        get_max_preds(merged)
    g_coords_r{0,1} [P, 17, 2]  the coords transform_preds was given, POST_PROCESS off / on
    g_preds_r{0,1} [P, 17, 2]   get_final_preds(merged, center, scale)
  neq_count, max_ulp            tests/test_heatmap_flip_cpu.py's heatmap_flip_decode_np against the four preds arrays: how many coordinates are not bit-equal, and
                                the largest distance in fp32 ulps
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from make_lift_golden import REF  # noqa: E402
from make_heatmap_golden import geometry, put, shim_missing_modules  # noqa: E402

F32 = np.float32
PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))       # COCO-17 left / right: flip_back's matched_parts


def partner():
    t = np.arange(17)
    for a, b in PAIRS:
        t[a], t[b] = b, a
    return t


def to_network_output(back):
    """Maps laid out as they should read after flip_back (before the shift) -> what the network gave for the mirrored crops: partner maps, columns reversed."""
    return np.ascontiguousarray(back[:, partner()][..., ::-1])


def merge_person(H, W):
    """17 hand-made map pairs in which the merge decides the outcome (tests/test_heatmap_flip_cpu.py reads this order).  d = the direct output; fb = the flipped
    output as it reads after flip_back: its column c lands on merged column c + 1 (column 0 also on column 0, column W - 1 nowhere)."""
    d, fb = np.zeros((17, H, W), F32), np.zeros((17, H, W), F32)
    m = H // 2
    d[0, 40, 20] = 0.25                                        # 0 (unpaired): the maximum exists only in the flipped operand
    put(fb[0], 9, W - 31, 1.0, left=0.5, right=0.25, up=0.25, down=0.5)
    put(d[1], 10, 30, 0.5, left=0.125, right=0.25, up=0.25, down=0.125)      # 1: two equal merged maxima, the first from the direct operand
    put(fb[1], 40, 19, 0.5, left=0.125, right=0.25, up=0.25, down=0.125)
    put(d[2], 50, 10, 0.5, left=0.125, right=0.25, up=0.25, down=0.125)      # 2: ... the first from the flipped operand
    put(fb[2], 12, 32, 0.5, left=0.25, right=0.125, up=0.125, down=0.25)
    fb[3, m, 0], fb[3, m, 1] = 1.0, 0.5                        # 3: the flipped map's edge column lands on merged columns 0 and 1: a tie, column 0 first
    d[4, m, 1], fb[4, m, 0] = 1.0, 0.5                         # 4: x = 1
    put(fb[5], m, W - 3, 1.0, left=0.25, right=0.5, up=0.125, down=0.5)      # 5: x = W - 2, refined from the flipped operand's neighbours
    fb[6, m, W - 2], fb[6, m, W - 3], fb[6, m, W - 1] = 1.0, 0.25, 2.0       # 6: x = W - 1; the 2.0 in the column the shift drops reaches nothing
    put(d[7], 30, 40, 1.0, left=0.5, right=0.25, up=0.125, down=0.5)         # 7: merged neighbours equal in x (0.5 + 0 = 0.25 + 0.25): sign(0) = 0
    fb[7, 30, 40] = 0.25
    d[8], fb[8] = -0.5, 0.25                                   # 8: the merged maximum is exactly zero: (0, 0)
    d[8, m, W // 2] = -0.25
    fb[9] = -1.0                                               # 9: the merged maximum is negative although the direct operand has a positive peak
    d[9, m, W // 2] = 0.5
    d[10, H - 14, 30], d[10, H - 14, 31] = 1.0, 0.75           # 10: peaks one column apart: the merged maximum is where the direct operand's is not
    fb[10, H - 14, 30], fb[10, H - 14, 29] = 1.0, 0.5
    put(d[11], 20, 15, 0.75, left=0.25, right=0.5, up=0.5, down=0.25)        # 11, 12: a pair whose operands disagree on the side: the flipped operand wins (11),
    put(fb[11], 60, W - 17, 1.0, left=0.25, right=0.5, up=0.5, down=0.25)
    put(d[12], 22, W - 20, 1.0, left=0.25, right=0.5, up=0.5, down=0.25)     # ... the direct operand wins (12)
    put(fb[12], 58, 18, 0.75, left=0.25, right=0.5, up=0.5, down=0.25)
    put(d[13], 2, 2, 1.0, left=0.25, right=0.5, up=0.5, down=0.25)           # 13: the first refined column and row, from the direct operand
    put(fb[14], H - 3, W - 4, 1.0, left=0.5, right=0.25, up=0.25, down=0.5)  # 14: the last refined column and row, from the flipped operand
    d[15, H - 20, 35], fb[15, H - 20, 34] = 0.5, 0.75          # 15: both operands peak on one merged pixel
    return d, fb                                               # 16: nothing anywhere


def blob_persons(g, P, H, W):
    """Gaussian blobs (sigma 1.5-3, amplitude 0.3-1, centers up to 2 px outside the map) on an exactly-zero background with noise in 1 % of the pixels; the
    flipped output's blob sits one column to the left of the direct one, give or take 0.7 px, with 0.8-1.1 of its amplitude."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)

    def one(cy, cx, s, amp):
        blob = amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        blob[blob < 0.01] = 0.0
        return blob + np.where(g.uniform(size=(H, W)) < 0.01, g.uniform(-0.05, 0.05, size=(H, W)), 0.0)

    d, fb = np.zeros((P, 17, H, W), np.float64), np.zeros((P, 17, H, W), np.float64)
    for p in range(P):
        for j in range(17):
            cy, cx = g.uniform(-2, H + 1), g.uniform(-2, W + 1)
            s, amp = g.uniform(1.5, 3.0), g.uniform(0.3, 1.0)
            d[p, j] = one(cy, cx, s, amp)
            fb[p, j] = one(cy + g.normal(0, 0.7), cx - 1 + g.normal(0, 0.7), s * g.uniform(0.9, 1.1), amp * g.uniform(0.8, 1.1))
    return d.astype(np.float16), fb.astype(np.float16)


def main():
    shim_missing_modules()
    sys.path.insert(0, os.path.join(REF, "demo"))
    from lib.hrnet.lib.utils import inference
    from lib.hrnet.lib.utils.transforms import flip_back
    from tests.test_heatmap_cpu import ulp_distance
    from tests.test_heatmap_flip_cpu import heatmap_flip_decode_np

    seen = []
    reference_transform = inference.transform_preds

    def recording_transform(coords, center, scale, output_size):
        seen.append(np.array(coords, copy=True))
        return reference_transform(coords, center, scale, output_size)

    inference.transform_preds = recording_transform
    g = np.random.default_rng(2026)
    out, neq, worst = {}, 0, 0
    for name, (H, W), (fw, fh) in (("a", (96, 72), (854, 480)), ("b", (64, 48), (8000, 4320))):
        d16, fb16 = blob_persons(g, 3, H, W)
        ed, efb = merge_person(H, W)
        hm16 = np.concatenate((d16, ed.astype(np.float16)[None]))
        back16 = np.concatenate((fb16, efb.astype(np.float16)[None]))
        assert np.array_equal(hm16[-1].astype(F32), ed) and np.array_equal(back16[-1].astype(F32), efb)
        hmf16 = to_network_output(back16)
        hm, hmf = hm16.astype(F32), hmf16.astype(F32)
        P = hm.shape[0]
        center, scale, _ = geometry(g, P, fw, fh)
        keep = hmf.copy()
        output_flipped = flip_back(hmf.copy(), [list(p) for p in PAIRS])                  # (flip_back writes into the array it is given)
        assert np.array_equal(output_flipped, back16.astype(F32)) and np.array_equal(hmf, keep)
        output_flipped[:, :, :, 1:] = output_flipped.copy()[:, :, :, 0:-1]
        merged = np.ascontiguousarray((hm + output_flipped) * 0.5)
        assert merged.dtype == F32
        maxpos, maxvals = inference.get_max_preds(merged.copy())
        out.update({f"{name}_hm": hm16, f"{name}_hmf": hmf16, f"{name}_center": center, f"{name}_scale": scale, f"{name}_merged": merged,
                    f"{name}_maxpos": maxpos, f"{name}_maxvals": maxvals})
        for r in (0, 1):
            cfg = types.SimpleNamespace(TEST=types.SimpleNamespace(POST_PROCESS=bool(r)))
            del seen[:]
            before = merged.copy()
            preds, mv = inference.get_final_preds(cfg, merged, center, scale)
            assert np.array_equal(merged, before) and np.array_equal(mv, maxvals) and preds.dtype == F32 and len(seen) == P
            out[f"{name}_preds_r{r}"] = preds
            out[f"{name}_coords_r{r}"] = np.stack(seen)
            mine = heatmap_flip_decode_np(hm16, hmf16, center, scale, refine=bool(r))
            dist = ulp_distance(mine[..., :2], preds)
            neq, worst = neq + int((dist != 0).sum()), max(worst, int(dist.max()))
    out["neq_count"], out["max_ulp"] = np.array(neq, np.int64), np.array(worst, np.int64)
    path = os.path.join(HERE, "heatmap_flip.npz")
    np.savez_compressed(path, **out)
    print("wrote heatmap_flip.npz:", {k: v.shape for k, v in out.items()}, "neq_count", neq, "max_ulp", worst, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
