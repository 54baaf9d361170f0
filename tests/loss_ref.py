"""The seven-term training loss restated in float64 torch from the formulas of include/kasf.h (kasf_loss7), with autograd for the gradient: what
tests/test_loss7_cpu.py ties to the fixture the reference's own utils/loss_calc.py wrote (tests/golden/make_loss7_golden.py) and what the host build of the
kernel (tests/test_loss_host_cpu.py) and the GPU tests (tests/test_gpu_loss7.py) are held to where the fixture has no number."""
import numpy as np
import torch

LIMBS = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14), (14, 15), (15, 16))
ANGLES = ((0, 3), (0, 6), (3, 6), (0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 10), (7, 13), (8, 13), (10, 13), (7, 8), (8, 9), (10, 11), (11, 12), (13, 14),
          (14, 15))
NAMES = ("total", "mpjpe", "n_mpjpe", "velocity", "limb_len_var", "limb_len", "cos_simi", "cos_simi_velocity")
DEFAULT_LAMBDAS = (0.5, 20.0, 0.0, 0.0, 0.0, 0.0)


def limb_vectors(x):
    a, b = [k[0] for k in LIMBS], [k[1] for k in LIMBS]
    return x[:, :, a] - x[:, :, b]                       # [B,T,16,3]


def limb_lengths(x):
    return limb_vectors(x).norm(dim=-1)                  # [B,T,16]


def limb_cosines(x):
    l = limb_vectors(x)
    u = l / l.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    i, j = [m[0] for m in ANGLES], [m[1] for m in ANGLES]
    return (u[:, :, i] * u[:, :, j]).sum(-1)             # [B,T,18]


def limb_angles(x):
    eps = 1e-7
    lo, hi = -1 + eps, 1 - eps
    if x.dtype == torch.float32:                          # a Python float against an fp32 tensor: the bound is rounded to fp32
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return torch.acos(limb_cosines(x).clamp(lo, hi))


def parts7(p, y):
    """The seven parts, each a 0-d tensor in p's dtype, in NAMES[1:] order."""
    zero = p.new_zeros(())
    T = p.shape[1]
    mpjpe = (p - y).norm(dim=-1).mean()
    s = (y * p).sum(dim=(2, 3), keepdim=True) / (p * p).sum(dim=(2, 3), keepdim=True)
    n_mpjpe = (s * p - y).norm(dim=-1).mean()
    vel = ((p[:, 1:] - p[:, :-1]) - (y[:, 1:] - y[:, :-1])).norm(dim=-1).mean() if T > 1 else zero
    lp, ly = limb_lengths(p), limb_lengths(y)
    var = lp.var(dim=1, unbiased=True).mean() if T > 1 else zero
    length = (lp - ly).abs().mean()
    tp, ty = limb_angles(p), limb_angles(y)
    cs = (tp - ty).abs().mean()
    cv = ((tp[:, 1:] - tp[:, :-1]) - (ty[:, 1:] - ty[:, :-1])).abs().mean() if T > 1 else zero
    return [mpjpe, n_mpjpe, vel, var, length, cs, cv]


def loss7_ref(pred, target, lambdas=DEFAULT_LAMBDAS, dtype=torch.float64, only=None):
    """(parts [8] numpy float64 laid out as NAMES, dtotal/dpred numpy in `dtype`).  only = an index into NAMES[1:]: total is that one part, unweighted."""
    p = torch.as_tensor(np.asarray(pred)).to(dtype).clone().requires_grad_(True)
    y = torch.as_tensor(np.asarray(target)).to(dtype)
    parts = parts7(p, y)
    if only is not None:
        total = parts[only]
    else:
        total = parts[0]
        for lam, part in zip(lambdas, parts[1:]):
            total = total + lam * part
    grad = torch.autograd.grad(total, p, allow_unused=True)[0] if total.requires_grad else None
    grad = torch.zeros_like(p) if grad is None else grad
    return np.array([float(total.detach())] + [float(v.detach()) for v in parts], np.float64), grad.detach().numpy()


def l1_arguments(pred, target):
    """Every argument of an L1 in the loss (length, angle and angle-velocity differences) and every cosine, float64: what the fixture keeps away from 0 and 1."""
    p, y = torch.as_tensor(np.asarray(pred)).double(), torch.as_tensor(np.asarray(target)).double()
    tp, ty = limb_angles(p), limb_angles(y)
    args = [(limb_lengths(p) - limb_lengths(y)).flatten(), (tp - ty).flatten()]
    if p.shape[1] > 1:
        args.append(((tp[:, 1:] - tp[:, :-1]) - (ty[:, 1:] - ty[:, :-1])).flatten())
    return torch.cat(args).abs().numpy(), torch.cat([limb_cosines(p).flatten(), limb_cosines(y).flatten()]).abs().numpy()


def rel_err(got, ref):
    """The project's measure (tests/gpu_util.py): largest difference over the reference's largest magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


def load_fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss7.npz"), allow_pickle=False)


def case_inputs(fx, name):
    """(pred, target) float32 [B,T,17,3] of a fixture case: the stored int16 times 2^-14, exact."""
    return tuple((fx[f"{name}_{k}"].astype(np.float32) * np.float32(2.0 ** -14)) for k in ("pred", "target"))


def case_runs(fx, regular_only=False):
    """[(case, lambda set name)] the fixture holds numbers for."""
    with_b = set(str(c) for c in fx["cases_B"])
    return [(str(c), s) for c in fx["cases"] for s in "AB" if (s == "A" or str(c) in with_b) and not (regular_only and str(c) == "special")]


TIE_CLIP, ZERO_LIMB_CLIP, COLLINEAR_CLIP = 0, 1, 2          # clips of the fixture's `special` case
