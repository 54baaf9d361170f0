#!/usr/bin/env python3
"""Generate the fixture of the person crop from the REAL reference helpers (run in the build container only).

    python tests/golden/make_crop_golden.py       # needs the reference checkout (make_lift_golden.REF)

Imports ``demo/lib/hrnet/lib/utils/utilitys.py`` for ``box_to_center_scale`` and ``demo/lib/hrnet/lib/utils/transforms.py`` for ``get_affine_transform`` and calls
them as they are, with make_heatmap_golden's in-process shim of the two modules that are not installed here (cv2: ``getAffineTransform`` only, solved with
``np.linalg.solve`` in float64; torchvision: empty).  ``cv2.warpAffine`` is NOT shimmed and nothing of a crop is recorded: there is no OpenCV build here to
record it from, so the sampling rules are tested against exact bilinear sampling instead (tests/test_crop_cpu.py).  ``ToTensor`` / ``Normalize`` are recorded
with torch's own CPU ops.  Writes tensors only:

  crop_persons.npz
    frames [2, 97, 400] uint8   two frames of 97 x 131 BGR pixels with a pitch of 400 bytes (the 7 padding bytes of each row are 255): 0 = smooth (sums of
                                sinusoids, adjacent-pixel difference <= 16), 1 = the same plus noise
    frame_hw [2], size [2]      int64: (97, 131); the crop's (width, height) = (24, 32)
    names [P], boxes [P, 4]     float32 x1, y1, x2, y2: inside the frame, over each edge, fully outside, larger than the frame, zero width, zero size, center
                                x == -1, a NaN, fractional corners, and "ties": a box whose crop positions fall exactly on half-grid ties in x and in y
    aspect                      float64 frame_height / frame_width, what the demo passes (utilitys.py:151)
    ref_center, ref_scale       box_to_center_scale(box as float64, frame_height, frame_width)
    ref_trans [P, 2, 3]         float64: get_affine_transform(center, scale, 0, size), the FORWARD matrix warpAffine is given; NaN where the shim's solve fails
    table_ref [3, 256]          float32: torch.arange(256, uint8).float().div(255).sub(mean[c]).div(std[c])
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from make_heatmap_golden import shim_missing_modules  # noqa: E402
from make_lift_golden import REF  # noqa: E402

F32, F64 = np.float32, np.float64
HF, WF, PITCH = 97, 131, 400
SIZE = (24, 32)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_frames():
    g = np.random.default_rng(2026)
    yy, xx = np.mgrid[0:HF, 0:WF].astype(F64)
    smooth = np.empty((HF, WF, 3), F64)
    for c, (fx, fy, ph) in enumerate(((0.11, 0.07, 0.3), (0.05, 0.13, 1.1), (0.09, 0.09, 2.0))):
        smooth[..., c] = 128 + 60 * np.sin(fx * xx + ph) * np.cos(fy * yy) + 50 * np.sin(0.04 * (xx + yy) + c)
    smooth = np.clip(np.rint(smooth), 0, 255)
    noisy = np.clip(smooth + g.integers(-90, 91, size=smooth.shape), 0, 255)
    buf = np.full((2, HF, PITCH), 255, np.uint8)
    for i, f in enumerate((smooth, noisy)):
        buf[i, :, :3 * WF] = f.astype(np.uint8).reshape(HF, 3 * WF)
    return buf


def ties_box(box_to_center_scale):
    """A box with center (60, 50) whose crop has kx = ky = 1025 / 2048 exactly: (kx x) 1024 is a half-integer for every odd x, (ky y + by) 1024 for every odd y."""
    from tests.test_crop_cpu import crop_geometry_np
    half = F32(9.609375 / 2)
    for _ in range(200000):
        box = np.array([F32(60) - half, 49, F32(60) + half, 51], F32)
        c, s = box_to_center_scale(box.astype(F64), HF, WF)
        kx, ky, bx, by = crop_geometry_np(c[None], s[None], *SIZE)
        if c[0] == 60 and c[1] == 50 and kx[0] == 1025 / 2048 and ky[0] == 1025 / 2048:
            return box
        half = np.nextafter(half, F32(0)) if kx[0] > 1025 / 2048 else np.nextafter(half, F32(100))
    raise SystemExit("no box with exact half-grid ties found")


def main():
    shim_missing_modules()
    sys.path.insert(0, os.path.join(REF, "demo"))
    from lib.hrnet.lib.utils.transforms import get_affine_transform
    from lib.hrnet.lib.utils.utilitys import box_to_center_scale

    persons = [("inside", (50, 30, 70, 60)), ("inside_wide", (30, 40, 90, 55)), ("left", (-10, 20, 15, 60)), ("right", (110, 30, 140, 70)),
               ("top", (40, -15, 70, 20)), ("bottom", (60, 70, 85, 110)), ("outside", (300, 300, 340, 380)), ("larger", (-40, -30, 180, 130)),
               ("zero_width", (65, 20, 65, 70)), ("center_x_minus_1", (-3, 10, 1, 40)), ("nan", (np.nan, 10, 50, 60)), ("ties", ties_box(box_to_center_scale)),
               ("zero_size", (64, 48, 64, 48)), ("fractional", (12.3, 7.7, 40.9, 66.1))]
    names = np.array([n for n, _ in persons])
    boxes = np.array([b for _, b in persons], F32)
    aspect = F64(HF) / F64(WF)
    centers, scales, trans = [], [], []
    for b in boxes:
        c, s = box_to_center_scale(b.astype(F64), HF, WF)          # (model_image_width, model_image_height) = shape[0], shape[1]
        assert c.dtype == s.dtype == F32
        try:
            with np.errstate(all="ignore"):
                m = np.asarray(get_affine_transform(c, s, 0, list(SIZE)), F64)
        except np.linalg.LinAlgError:
            m = np.full((2, 3), np.nan)
        centers.append(c), scales.append(s), trans.append(m)
    v = torch.arange(256, dtype=torch.uint8)
    table = np.stack([v.float().div(255).sub(MEAN[c]).div(STD[c]).numpy() for c in range(3)])
    out = dict(frames=make_frames(), frame_hw=np.array([HF, WF], np.int64), size=np.array(SIZE, np.int64), names=names, boxes=boxes, aspect=aspect,
               ref_center=np.stack(centers), ref_scale=np.stack(scales), ref_trans=np.stack(trans), table_ref=table)
    path = os.path.join(HERE, "crop_persons.npz")
    np.savez_compressed(path, **out)
    print("wrote crop_persons.npz:", {k: a.shape for k, a in out.items()}, os.path.getsize(path), "bytes;",
          "forward matrices that exist:", int(np.isfinite(out["ref_trans"]).all(axis=(1, 2)).sum()), "of", len(persons))


if __name__ == "__main__":
    main()
