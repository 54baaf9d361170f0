#!/usr/bin/env python3
"""Generate the fixture of the detector's letterbox from the REAL reference functions (run in the build container only).

    python tests/golden/make_letterbox_golden.py       # needs the reference checkout (make_lift_golden.REF)

Imports ``demo/lib/yolov3/preprocess.py`` and calls its ``letterbox_image`` and ``prep_image`` as they are.  The ``cv2`` they import is not installed here and
is replaced IN THIS PROCESS ONLY by a stand-in module whose ``resize`` is this project's numpy restatement of the resampling (tests/test_letterbox_cpu.py,
``resize_cubic_np``: include/kasf.h rules 2-3).  THE RESAMPLING ARITHMETIC IS THIS PROJECT'S RESTATEMENT, not OpenCV's code: the fixture pins the reference's
bookkeeping -- ``new_w`` / ``new_h`` as it computes them, the placement on the canvas, the canvas of 128, the ``[:, :, ::-1]`` reversal, the layout and
``float().div(255.0)`` -- around that resampling.  The stand-in asserts that it is called with ``interpolation=INTER_CUBIC`` and records every ``dsize`` it is
given.  ``PIL`` is imported by the module for ``prep_image_pil`` only, which is not called: an empty stand-in when it is missing.  Writes tensors only:

  letterbox.npz
    land_buf [97, 400] uint8, land_hw = (97, 131)        a smooth landscape frame behind a padded pitch (padding bytes 255); pixel (y, x, c) = buf[y, 3 x + c]
    port_buf [131, 304] uint8, port_hw = (131, 97)       a noisy portrait frame, the same way
    {land,port}_prep_{64,32} [1, 3, d, d] float32        prep_image(frame, d)[0]
    land_canvas_48x32 [32, 48, 3] uint8                  letterbox_image(frame, (48, 32)) (the reference's canvas is int64; every value fits a byte, asserted)
    calls [n] str "frame:w:h", dsize [n, 2] int32        what cv2.resize was asked for in each of those calls: (new_w, new_h)
    placement [n, 4] int32                               pad_x, pad_y, new_w, new_h: the box of non-128 pixels of letterbox_image on a frame of 7s
    interpolation int32                                  the stand-in's INTER_CUBIC (2, OpenCV's value)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from make_lift_golden import REF  # noqa: E402
from tests.test_letterbox_cpu import resize_cubic_np  # noqa: E402

INTER_CUBIC = 2
DSIZES = []


def resize(img, dsize, interpolation=None):
    assert interpolation == INTER_CUBIC, "the reference asks for INTER_CUBIC"
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3
    DSIZES.append((int(dsize[0]), int(dsize[1])))
    return resize_cubic_np(img, int(dsize[0]), int(dsize[1]))


def shim_missing_modules():
    cv2 = types.ModuleType("cv2")
    cv2.resize, cv2.INTER_CUBIC = resize, INTER_CUBIC
    sys.modules["cv2"] = cv2
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        sys.modules["PIL"] = types.ModuleType("PIL")
        sys.modules["PIL.Image"] = sys.modules["PIL"].Image = types.ModuleType("PIL.Image")
        print("shimmed PIL")


def pitched(frame, pitch):
    buf = np.full((frame.shape[0], pitch), 255, np.uint8)
    buf[:, :3 * frame.shape[1]] = frame.reshape(frame.shape[0], -1)
    return buf


def frames():
    g = np.random.default_rng(20261018)
    yy, xx = np.mgrid[0:97, 0:131].astype(np.float64)
    land = np.stack([128 + 70 * np.sin(0.045 * xx + c) * np.cos(0.06 * yy) + 40 * np.sin(0.03 * (xx + yy) + 2 * c) for c in range(3)], axis=-1)
    return {"land": np.clip(np.rint(land), 0, 255).astype(np.uint8), "port": g.integers(0, 256, (131, 97, 3)).astype(np.uint8)}


def main():
    shim_missing_modules()
    sys.path.insert(0, os.path.join(REF, "demo"))
    from lib.yolov3 import preprocess as ref

    fr = frames()
    out = {"land_buf": pitched(fr["land"], 400), "land_hw": np.array([97, 131], np.int32), "port_buf": pitched(fr["port"], 304),
           "port_hw": np.array([131, 97], np.int32), "interpolation": np.int32(INTER_CUBIC)}
    calls, dsize, placement = [], [], []

    def record(name, w, h):
        calls.append(f"{name}:{w}:{h}")
        dsize.append(DSIZES[-1])
        marker = ref.letterbox_image(np.full_like(fr[name], 7), (w, h))
        DSIZES.pop()
        ys, xs = np.nonzero((marker != 128).any(axis=-1))
        placement.append((xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1))

    for name in ("land", "port"):
        for dim in (64, 32):
            t, orig, wh = ref.prep_image(fr[name], dim)
            assert orig is fr[name] and tuple(wh) == (fr[name].shape[1], fr[name].shape[0]) and tuple(t.shape) == (1, 3, dim, dim)
            out[f"{name}_prep_{dim}"] = t.numpy()
            record(name, dim, dim)
    canvas = ref.letterbox_image(fr["land"], (48, 32))
    assert canvas.shape == (32, 48, 3) and canvas.min() >= 0 and canvas.max() <= 255
    out["land_canvas_48x32"] = canvas.astype(np.uint8)
    record("land", 48, 32)
    out.update(calls=np.array(calls), dsize=np.array(dsize, np.int32), placement=np.array(placement, np.int32))
    assert len(DSIZES) == len(calls)
    path = os.path.join(HERE, "letterbox.npz")
    np.savez_compressed(path, **out)
    assert not any(v.dtype == object for v in out.values())
    print("wrote letterbox.npz:", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
