"""Operands and the reference of the input-gradient kernel (csrc/k_input_grad.hip; include/kasf.h, kasf_op_input_grad), shared by tests/test_input_grad_cpu.py,
tests/test_input_grad_host_cpu.py and tests/test_gpu_input_grad.py.  Nothing here needs a GPU.

`input_grad_ref` is the closed-form rule written out by hand in torch and evaluated in the dtype of its operands, as tests/misc_ref.py does: fp64 gives the
reference, fp32 gives "a plain fp32 evaluation of the same formulas" whose distance from the fp64 one is the sensitivity the fp32 bar is 8 x of.  The CPU test
holds the rule itself to torch autograd through oracle.bone_decompose, oracle._BoneRefusion and the three embeddings.
"""
import functools

import torch

from oracle import kasf_oracle as O
from tests import misc_ref as R

J = 17
# The launch walks frames four at a time (one wavefront each) on at most 512 workgroups: a workgroup's second walk starts at frame 2,048 and its third at 4,096 --
# where misc_ref.prologue_x plants its zero-length bones (frames 0, 2048, 4096) and all-zero frames (2, 2050, 4098) again.
FRAMES = (1, 3, 2049, 4100)
SECOND_WALK = 2048
PATHS = {"joints": (True, False, False), "bones": (False, True, False), "limbs": (False, False, True), "all": (True, True, True)}
_CH = ("mlp_dir_x", "mlp_dir_y", "mlp_len")

# The fp32 bar: 8 x the measured sensitivity, rounded UP to one digit.  Sensitivity = frame_err(fp32 evaluation of input_grad_ref, its fp64 evaluation) at the
# largest shape (4,100 frames), the worst of the four operand sets of PATHS: measured 1.7e-6 ("bones"; "all" 1.3e-6, "limbs" 4.5e-7, "joints" 0; at 3 frames
# 1.3e-7) -> 8 x 1.7e-6 = 1.4e-5 -> 2e-5.  tests/test_input_grad_cpu.py::test_fp32_sensitivity_is_within_the_bar re-measures it on every run; DESIGN.md 7.2.
BAR32 = 2e-5


def frame_err(got, ref):
    """Per frame max |got - ref| over the frame's own largest |ref|, the worst over the frames (a whole-array measure would hide everything behind the one
    bone 0.0027 long of prologue_x(4100), whose gradient is 100 x any other value).  A frame whose reference is all zero must be all zero."""
    got, ref = got.detach().double().reshape(-1, J * 3), ref.detach().double().reshape(-1, J * 3)
    diff, mx = (got - ref).abs().amax(1), ref.abs().amax(1)
    err = torch.where(mx > 0, diff / mx.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    return float(err.max())


@functools.lru_cache(maxsize=None)
def inputs(frames):
    """x = misc_ref.prologue_x(frames) and three seeded randn gradients a (joints_embed input), b (bone3), c (limb3), all [frames,17,3] fp32"""
    g = R.gen(8, frames)
    return dict(x=R.prologue_x(frames), a=torch.randn(frames, J, 3, generator=g), b=torch.randn(frames, J, 3, generator=g), c=torch.randn(frames, J, 3, generator=g))


def picked(i, path):
    """(a, b, c) of `inputs` with the paths PATHS[path] leaves out as None"""
    return tuple(i[n] if use else None for n, use in zip("abc", PATHS[path]))


def input_grad_ref(x, a, b, c, P):
    """x [F,17,3]; a, b, c [F,17,3] or None (= zero); P name -> tensor (the limb-MLP parameters), all of one dtype -> dx [F,17,3] in that dtype"""
    dx = torch.zeros_like(x)
    if a is not None:                                   # 1. joints: the embedding reads x itself
        dx = dx + a
    if b is not None:                                   # 2. bones (KASportsFormer.py:42-62)
        child, parent = torch.tensor(O.BONE_CHILD), torch.tensor(O.BONE_PARENT)
        bp = b[:, :16] + b[:, 16:17] / 16               # row 16 of bone3 is the mean of rows 0..15
        v = x[:, child, :2] - x[:, parent, :2]
        ln = torch.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])
        nz = (ln != 0)[..., None]
        safe = torch.where(nz, ln[..., None], torch.ones_like(ln[..., None]))
        u = v / safe
        gv = (bp[..., :2] - u * (u * bp[..., :2]).sum(-1, keepdim=True)) / safe + bp[..., 2:3] * u
        gv = torch.where(nz, gv, bp[..., :2])           # zero length: the forward used the constant 1, the length column contributes nothing
        xy = torch.zeros_like(x[..., :2])
        xy.index_add_(1, child, gv)
        xy.index_add_(1, parent, -gv)
        dx = dx + torch.cat((xy, torch.zeros_like(x[..., 2:])), dim=-1)
    if c is not None:                                   # 3. the 51 limb MLPs on the raw joints (bone_refusion.py, bone_MLP.py)
        add = torch.zeros_like(x)
        for i, grp in enumerate(O.LIMB_GROUPS):
            for ch, name in enumerate(_CH):
                pre = f"bone_refusion.mlp_layers.{i}.{name}."
                w1, b1, w2 = P[pre + "fc1.weight"], P[pre + "fc1.bias"], P[pre + "fc2.weight"]
                z = x[:, list(grp), ch] @ w1.T + b1                               # [F,16]
                dgelu = 0.5 * (1 + torch.erf(z * 0.5 ** 0.5)) + z * torch.exp(-0.5 * z * z) * (0.5 / torch.pi) ** 0.5
                add[:, list(grp), ch] += (c[:, i, ch:ch + 1] * w2 * dgelu) @ w1      # a group never names a joint twice
        dx = dx + add
    return dx


def limb_params(P, dtype):
    return {n: t.to(dtype) for n, t in P.items() if n.startswith("bone_refusion.")}


def reference64(frames, path, P):
    i = inputs(frames)
    a, b, c = picked(i, path)
    d = lambda t: None if t is None else t.double()
    return input_grad_ref(i["x"].double(), d(a), d(b), d(c), limb_params(P, torch.float64))


def measure_fp32_sensitivity(P, frames=max(FRAMES)):
    """path -> frame_err(fp32 evaluation, fp64 evaluation) of input_grad_ref on the same fp32-representable operands"""
    i = inputs(frames)
    out = {}
    for path in PATHS:
        a, b, c = picked(i, path)
        out[path] = frame_err(input_grad_ref(i["x"], a, b, c, limb_params(P, torch.float32)), reference64(frames, path, P))
    return out
