#!/usr/bin/env python3
"""Generate the lifting fixtures from the REAL reference demo (run in the build container only).

    python tests/golden/make_lift_golden.py          # needs the reference checkout (see make_golden.import_reference)

Imports ``demo/demo.py`` for its ``resample`` / ``turn_into_clips`` (demo.py:132-156) and ``demo/lib/utils.py`` for
``normalize_screen_coordinates`` / ``flip_data``; the detector, video and plotting imports the demo drags in get inert stand-ins
(``cv2``, ``tqdm``, ``lib.hrnet.gen_kpts``, ``lib.preprocess``, ``model.model_tools``, ``easydict``).  Writes tensors only:

  lift_tables.npz   resample(L, T) and first_pos (= np.unique(r, return_index=True)[1]) for L in 1..T-1, T in {27, 81, 243}
                    (rows padded with -1)
  lift_e2e.npz      float32 pixel tracks at 1280 x 720 with confidences and the demo's lift of each (its per-clip loop, lift_3d_pose,
                    demo.py:222-236): the real reference model, 2 layers, 8 heads, T = 27, eval mode, weights from
                    oracle.name_seeded_fill -- with ``flip_data`` applied to a COPY (demo.py:227 flips the clip in place).
                    N = 54 = 2 T: turn_into_clips raises UnboundLocalError there; its expected output is built from the two full clips directly.
                    sens_* [P, N]: per frame, how far the reference's own lift moves when the pixel track carries 1e-6 relative noise.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import import_reference  # noqa: E402
from oracle import kasf_oracle as O  # noqa: E402

REF = "/root/reference"
W_PX, H_PX, T = 1280, 720, 27
CASES_N = (1, 20, 27, 54, 61)


def import_demo():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class EasyDict(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    mod("cv2")
    mod("tqdm", tqdm=lambda it, *a, **k: it)
    mod("lib.hrnet.gen_kpts", gen_video_kpts=None)
    mod("lib.preprocess", h36m_coco_format=None)
    mod("model.model_tools", load_model=None)
    mod("easydict", EasyDict=EasyDict)
    sys.path.insert(0, os.path.join(REF, "demo"))
    import demo
    return demo


def tables():
    demo = import_demo()
    out = {}
    for t in (27, 81, 243):
        r = np.full((t - 1, t), -1, np.int32)
        fp = np.full((t - 1, t - 1), -1, np.int32)
        for L in range(1, t):
            idx = demo.resample(L, t)
            r[L - 1] = idx
            u = np.unique(idx, return_index=True)[1]
            assert len(u) == L
            fp[L - 1, :L] = u
        out[f"resample_T{t}"], out[f"first_pos_T{t}"] = r, fp
    np.savez_compressed(os.path.join(HERE, "lift_tables.npz"), **out)
    print("wrote lift_tables.npz")
    return demo


def track(P, N, seed):
    """Smooth pixel tracks inside the frame: a per-person skeleton offset plus a slow drift and jitter, confidences in [0.3, 1]."""
    g = np.random.default_rng(seed)
    base = g.uniform((300, 150), (980, 570), size=(P, 1, 17, 2))
    drift = np.cumsum(g.normal(0, 4, size=(P, N, 1, 2)), axis=1)
    xy = base + drift + g.normal(0, 2, size=(P, N, 17, 2))
    conf = g.uniform(0.3, 1.0, size=(P, N, 17, 1))
    return np.concatenate((xy, conf), axis=-1).astype(np.float32)


def _tta_clip(model, clip_px):
    """One clip [P, T, 17, 3] of pixels -> the flip-averaged prediction with the root joint at zero, built from the demo's own helpers
    (normalize_screen_coordinates, flip_data) with the mirror taken of a COPY of the normalised clip."""
    from lib.utils import normalize_screen_coordinates, flip_data
    views = normalize_screen_coordinates(clip_px, w=W_PX, h=H_PX).astype(np.float32)
    with torch.no_grad():
        plain = model(torch.from_numpy(views))
        unmirrored = flip_data(model(torch.from_numpy(flip_data(views.copy()))))
    merged = ((plain + unmirrored) / 2).numpy()
    merged[:, :, 0, :] = 0
    return merged


def demo_lift(demo, model, keypoints):
    """The demo's lift of a [P, N, 17, 3] track (lift_3d_pose's per-clip loop, demo.py:222-236): the clips of turn_into_clips, one TTA
    prediction each, the last one reduced to its original frames through the returned downsample index."""
    clips, keep = demo.turn_into_clips(keypoints, T)
    preds = [_tta_clip(model, c) for c in clips]
    preds[-1] = preds[-1][:, keep]
    return np.concatenate(preds, axis=1)


def full_clip_lift(demo, model, keypoints):
    """N = k T: the clips the demo would build if turn_into_clips did not raise (every clip full, nothing downsampled)."""
    return np.concatenate([_tta_clip(model, keypoints[:, a:a + T]) for a in range(0, keypoints.shape[1], T)], axis=1)


def sensitivity(fn, demo, model, kp, lift):
    """[P, N] per frame: the largest change of the reference's lift, relative to the lift's scale, over eight lifts of the pixel track
    perturbed by 1e-6 relative noise (a few float32 ulps; the repeated frames of a resampled clip stay identical copies).  Near-ties in the
    temporal GCN's top-k (graph.py:104-112) make some windows of this random-weight model ill-conditioned."""
    d = np.zeros(lift.shape[:2])
    for seed in range(8):
        g = np.random.default_rng(seed)
        q = fn(demo, model, (kp * (1 + 1e-6 * g.standard_normal(kp.shape))).astype(np.float32))
        d = np.maximum(d, np.abs(q - lift).max(axis=(2, 3)) / np.abs(lift).max())
    return d.astype(np.float32)


def main():
    Ref, _, _, _ = import_reference()
    torch.set_num_threads(8)
    demo = tables()
    model = Ref(n_layers=2, dim_in=3, dim_feat=128, dim_rep=512, dim_out=3, mlp_ratio=4, num_heads=8, n_frames=T)
    model.load_state_dict(O.name_seeded_fill(model.state_dict()), strict=True)
    model.eval()
    out = {"width": np.array(W_PX), "height": np.array(H_PX), "T": np.array(T), "n_layers": np.array(2),
           "note": np.array("lift_n54: turn_into_clips raises UnboundLocalError at N = 2T; expected output built from the two full clips")}
    for k, n in enumerate(CASES_N):
        kp = track(1, n, seed=100 + k)
        kp_in = kp.copy()
        if n > T and n % T == 0:
            try:
                demo.turn_into_clips(kp, T)
                raise AssertionError("turn_into_clips was expected to raise at N = k T")
            except UnboundLocalError:
                pass
            fn = full_clip_lift
        else:
            fn = demo_lift
        lift = fn(demo, model, kp)
        assert np.array_equal(kp, kp_in) and lift.shape == (1, n, 17, 3)
        out[f"track_n{n}"], out[f"lift_n{n}"], out[f"sens_n{n}"] = kp[0], lift[0], sensitivity(fn, demo, model, kp, lift)[0]
    kp = track(2, 40, seed=200)
    out["track_p2"], out["lift_p2"] = kp, demo_lift(demo, model, kp)
    out["sens_p2"] = sensitivity(demo_lift, demo, model, kp, out["lift_p2"])
    assert out["lift_p2"].shape == (2, 40, 17, 3)
    np.savez_compressed(os.path.join(HERE, "lift_e2e.npz"), **out)
    print("wrote lift_e2e.npz:", {k: v.shape for k, v in out.items() if v.ndim})


if __name__ == "__main__":
    main()
