#!/usr/bin/env python3
"""Generate the fixture of the seven-term training loss from the REAL reference functions (run in the build container only).

    python tests/golden/make_loss7_golden.py       # needs the reference checkout (make_lift_golden.REF)

Imports the reference's ``utils/loss_calc.py`` as it is and combines its seven functions as ``train_and_evaluate_sp.py:216-220`` spells out
``loss_total_complete``; ``dtotal/dpred`` is torch autograd through them.  Writes numbers only:

  loss7.npz
    lambdas_A, lambdas_B [6]    {n_mpjpe, velocity, limb_len_var, limb_len, limb_cos_simi, limb_cos_simi_velocity}; B has one new lambda set (the yaml experiment)
    cases, cases_B              names of the cases; of those that also carry set B
    <case>_pred, <case>_target  int16 [B,T,17,3]: the value is q * 2^-14 exactly (target ~ 0.3 N(0,1), pred = target + 0.05 N(0,1), rounded to that grid:
                                every input is an exact fp32 number, and the file stays small)
    <case>_parts64_<S>  [8]     float64 {total, mpjpe, n_mpjpe, velocity, limb_len_var, limb_len, cos_simi, cos_simi_velocity} by the reference on float64 inputs
    <case>_grad64_<S>           float64 [B,T,17,3] dtotal/dpred, the same run
    <case>_parts32_<S>  [8]     the reference on float32 inputs: the yardstick for margins
    <case>_graderr32_<S>        rel_err (largest difference / largest magnitude) of the float32 run's gradient against the float64 one
  Regular cases r3x27, r2x2, r2x1, r1x81, r1x243, r300x3: the generator draws frames again (draw_regular) until every L1 argument (length, angle and
  angle-velocity differences) has magnitude >= 1e-5 and every |cosine| <= 0.999 -- the sign and 1 / sqrt(1 - c^2) make the gradient discontinuous or
  ill-conditioned near those points.
  The case `special` [3,9,17,3] holds three clips: 0 the tie clip (pred == target), 1 a zero-length limb (pred joint 2 = pred joint 1 in every frame),
  2 two exactly collinear limbs (pred joints 0, 1, 2 on one line in every frame: the clamp is active).
The float64 restatement tests/loss_ref.py is asserted against the reference here as well, special clips included.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from make_lift_golden import REF  # noqa: E402
from tests import loss_ref  # noqa: E402

SCALE = 2.0 ** -14
LAMBDAS = {"A": (0.5, 20.0, 0.5, 0.25, 0.1, 0.2), "B": (0.5, 20.0, 0.0, 0.1, 0.0, 0.0)}
REGULAR = (("r3x27", 3, 27), ("r2x2", 2, 2), ("r2x1", 2, 1), ("r1x81", 1, 81), ("r1x243", 1, 243), ("r300x3", 300, 3))
WITH_B = ("r3x27", "r2x2", "r2x1", "r1x81", "special")


def import_loss_calc():
    sys.path.insert(0, REF)
    import utils.loss_calc as LC
    return LC


def draw(B, T, seed):
    g = np.random.RandomState(seed)
    target = np.round(0.3 * g.standard_normal((B, T, 17, 3)) / SCALE)
    pred = np.round((target * SCALE + 0.05 * g.standard_normal((B, T, 17, 3))) / SCALE)
    assert np.abs(pred).max() < 32767 and np.abs(target).max() < 32767
    return pred.astype(np.int16), target.astype(np.int16)


def reference(LC, pred_q, target_q, lambdas, dtype):
    p = torch.tensor(pred_q.astype(np.float64) * SCALE, dtype=dtype, requires_grad=True)
    y = torch.tensor(target_q.astype(np.float64) * SCALE, dtype=dtype)
    parts = [LC.mpjpe_loss_calc(p, y), LC.n_mpjpe_loss_calc(p, y), LC.velocity_loss_calc(p, y), LC.loss_limb_var_calc(p), LC.loss_limb_len_calc(p, y),
             LC.loss_cos_simi_calc(p, y), LC.loss_cos_simi_velocity_calc(p, y)]
    total = parts[0]
    for lam, part in zip(lambdas, parts[1:]):
        total = total + lam * part
    total.backward()
    return np.array([float(total.detach())] + [float(v.detach()) for v in parts], np.float64), p.grad.numpy().astype(np.float64)


def irregular_frames(pred_q, target_q):
    """[B,T] bool: frames that hold an L1 argument below 1e-5 or a |cosine| above 0.999 (a velocity argument marks both of its frames)."""
    p, y = (torch.tensor(a.astype(np.float64) * SCALE) for a in (pred_q, target_q))
    tp, ty = loss_ref.limb_angles(p), loss_ref.limb_angles(y)
    bad = ((loss_ref.limb_lengths(p) - loss_ref.limb_lengths(y)).abs() < 1e-5).any(-1) | ((tp - ty).abs() < 1e-5).any(-1)
    bad |= (loss_ref.limb_cosines(p).abs() > 0.999).any(-1) | (loss_ref.limb_cosines(y).abs() > 0.999).any(-1)
    if p.shape[1] > 1:
        w = (((tp[:, 1:] - tp[:, :-1]) - (ty[:, 1:] - ty[:, :-1])).abs() < 1e-5).any(-1)
        bad[:, :-1] |= w
        bad[:, 1:] |= w
    return bad.numpy()


def draw_regular(B, T, seed):
    """draw(), then the irregular frames drawn again -- a seed search frame by frame: one |cosine| in a thousand lies above 0.999, so no whole draw of more than
    a few hundred angles passes -- until none is left."""
    pred, target = draw(B, T, seed)
    g = np.random.RandomState(seed + 1)
    for rounds in range(1000):
        bad = irregular_frames(pred, target)
        if not bad.any():
            args, cosines = loss_ref.l1_arguments(pred.astype(np.float64) * SCALE, target.astype(np.float64) * SCALE)
            assert args.min() >= 1e-5 and cosines.max() <= 0.999
            return pred, target, rounds
        n = int(bad.sum())
        t = np.round(0.3 * g.standard_normal((n, 17, 3)) / SCALE)
        target[bad] = t.astype(np.int16)
        pred[bad] = np.round((t * SCALE + 0.05 * g.standard_normal((n, 17, 3))) / SCALE).astype(np.int16)
    raise SystemExit("no regular draw")


def special():
    pred, target = draw(3, 9, 99)
    pred[0] = target[0]                                  # the tie clip
    pred[1, :, 2] = pred[1, :, 1]                        # a zero-length limb (1 -> 2)
    step = (pred[2, :, 1].astype(np.int32) - pred[2, :, 0]) // 2
    pred[2, :, 1] = pred[2, :, 0] + step                 # joints 0, 1, 2 on one line: limbs 0 and 1 are exactly collinear (angle (0, 1))
    pred[2, :, 2] = pred[2, :, 1] + 2 * step
    assert (step != 0).any(axis=-1).all()
    return pred, target


def main():
    LC = import_loss_calc()
    out = {"lambdas_A": np.array(LAMBDAS["A"], np.float64), "lambdas_B": np.array(LAMBDAS["B"], np.float64),
           "cases": np.array([c[0] for c in REGULAR] + ["special"]), "cases_B": np.array(WITH_B)}
    inputs = {}
    for name, B, T in REGULAR:
        pred, target, rounds = draw_regular(B, T, 1000 * B + T)
        print(f"{name}: regular after {rounds} rounds of redrawn frames")
        inputs[name] = (pred, target)
    inputs["special"] = special()
    for name, (pred, target) in inputs.items():
        out[name + "_pred"], out[name + "_target"] = pred, target
        for S, lam in LAMBDAS.items():
            if S == "B" and name not in WITH_B:
                continue
            parts64, grad64 = reference(LC, pred, target, lam, torch.float64)
            parts32, grad32 = reference(LC, pred, target, lam, torch.float32)
            assert np.isfinite(parts64).all() and np.isfinite(grad64).all() and np.isfinite(grad32).all(), name
            rparts, rgrad = loss_ref.loss7_ref(pred.astype(np.float64) * SCALE, target.astype(np.float64) * SCALE, lam)
            assert np.abs(rparts - parts64).max() < 1e-12 and loss_ref.rel_err(rgrad, grad64) < 1e-10, (name, S, "the restatement is not the reference")
            err32 = loss_ref.rel_err(grad32, grad64)
            print(f"{name} {S}: fp32 reference vs fp64: parts {np.abs(parts32 - parts64).max():.2e}, gradient rel_err {err32:.2e}")
            out[f"{name}_parts64_{S}"], out[f"{name}_grad64_{S}"] = parts64, grad64
            out[f"{name}_parts32_{S}"], out[f"{name}_graderr32_{S}"] = parts32, np.float64(err32)
    path = os.path.join(HERE, "loss7.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
