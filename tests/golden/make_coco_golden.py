#!/usr/bin/env python3
"""Generate the fixture of the lift's two ends from the REAL reference demo helpers (run in the build container only).

    python tests/golden/make_coco_golden.py          # needs the reference checkout (make_lift_golden.REF)

Imports ``demo/lib/preprocess.py`` for ``h36m_coco_format`` (the file demo.py imports: spine factor 2) and ``demo/lib/utils.py`` for
``camera_to_world``; the three lines after it in the demo (demo.py:245-248) are applied as written there.  Writes tensors only:

  coco_world.npz
    coco [P, N, 17, 3]          float32 COCO-17 pixel x, y, score (P = 3, N = 61): coordinates from sub-pixel to 4,000 px, one all-zero frame
                                inside track 1
    h36m_kpts [P, N, 17, 2],    what h36m_coco_format(coco[..., :2], coco[..., 2]) returns (no person is all zero, so P is kept)
    h36m_scores [P, N, 17]
    rot [4], t [3]              demo.py:243's quaternion; a non-zero translation for the camera_to_world-only case
    for each camera-space input X in lift_e2e.npz's lift_n61 [61, 17, 3] and lift_p2 [2, 40, 17, 3]:
      post_X                    the demo's post_out for every frame: camera_to_world(frame, rot, 0), z -= min z, /= max (demo.py:245-248)
      c2w_X                     camera_to_world(frame, rot, t) alone
    world_err_ref               the largest |reference fp32 result - float64 evaluation of the same formula| over all post_* and c2w_* values
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_lift_golden import REF  # noqa: E402

P, N = 3, 61
T_VEC = np.array([0.25, -0.5, 1.0], np.float32)


def coco_tracks():
    """[P, N, 17, 3]: person 0 an ordinary 1280 x 720 track, person 1 a 4K frame with one all-zero frame, person 2 sub-pixel to a few pixels, and a
    few joints of every person scaled across magnitudes; scores in [0, 1]."""
    g = np.random.default_rng(2024)
    scale = np.array([1280.0, 4000.0, 4.0])[:, None, None, None]
    xy = g.uniform(0, 1, size=(P, N, 17, 2)) * scale
    xy *= 10.0 ** g.integers(-3, 1, size=(P, N, 17, 1))        # each joint 1x, 0.1x, 0.01x or 0.001x: sub-pixel values in every track
    score = g.uniform(0, 1, size=(P, N, 17, 1))
    coco = np.concatenate((xy, score), axis=-1).astype(np.float32)
    coco[1, 30] = 0
    return coco


def world_f64(x, rot, t, floor, unit):
    """The float64 evaluation of qrot's formula plus t, the floor and the unit step on float32 inputs [..., 17, 3]."""
    v, q, t = x.astype(np.float64), rot.astype(np.float64), np.asarray(t, np.float64)
    qv = np.broadcast_to(q[1:], v.shape)
    uv = np.cross(qv, v)
    uuv = np.cross(qv, uv)
    out = v + 2 * (q[0] * uv + uuv) + t
    if floor:
        out[..., 2] -= out[..., 2].min(axis=-1, keepdims=True)
    if unit:
        out /= out.max(axis=(-2, -1), keepdims=True)
    return out


def main():
    sys.path.insert(0, os.path.join(REF, "demo"))
    from lib.preprocess import h36m_coco_format
    from lib.utils import camera_to_world

    out = {}
    coco = coco_tracks()
    keep = coco.copy()
    kpts, scores, _ = h36m_coco_format(coco[..., :2], coco[..., 2])
    assert np.array_equal(coco, keep)
    assert kpts.shape == (P, N, 17, 2) and scores.shape == (P, N, 17) and kpts.dtype == scores.dtype == np.float32
    assert not kpts[1, 30].any() and not scores[1, 30].any() and kpts[1, 29].any()
    out["coco"], out["h36m_kpts"], out["h36m_scores"] = coco, kpts, scores

    rot = np.array([0.1407056450843811, -0.1500701755285263, -0.755240797996521, 0.6223280429840088], dtype="float32")   # demo.py:243-244
    out["rot"], out["t"] = rot, T_VEC
    lifts = np.load(os.path.join(HERE, "lift_e2e.npz"), allow_pickle=False)
    err = 0.0
    for name in ("lift_n61", "lift_p2"):
        x = lifts[name]
        frames = x.reshape(-1, 17, 3)
        post, c2w = np.empty_like(frames), np.empty_like(frames)
        for j, frame in enumerate(frames):
            post_out = camera_to_world(frame.copy(), R=rot, t=0)                # demo.py:245-248
            post_out[:, 2] -= np.min(post_out[:, 2])
            max_value = np.max(post_out)
            post_out /= max_value
            post[j] = post_out
            c2w[j] = camera_to_world(frame.copy(), R=rot, t=T_VEC)
        assert post.dtype == c2w.dtype == np.float32
        err = max(err, np.abs(post - world_f64(frames, rot, 0.0, True, True)).max(), np.abs(c2w - world_f64(frames, rot, T_VEC, False, False)).max())
        out["post_" + name], out["c2w_" + name] = post.reshape(x.shape), c2w.reshape(x.shape)
    out["world_err_ref"] = np.array(err, np.float64)
    np.savez_compressed(os.path.join(HERE, "coco_world.npz"), **out)
    print("wrote coco_world.npz:", {k: v.shape for k, v in out.items()}, "world_err_ref", err, os.path.getsize(os.path.join(HERE, "coco_world.npz")), "bytes")


if __name__ == "__main__":
    main()
