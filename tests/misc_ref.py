"""Operands and references of tests/test_gpu_misc.py (the kernels of csrc/k_misc.hip on their own), kept apart from the GPU tests so that the CPU suite can
measure what the bars are derived from (tests/test_misc_ops_cpu.py).

Every reference is plain torch math on the operands AS THE KERNEL SEES THEM (already rounded to the storage dtype), written once and evaluated in the dtype of
its operands: fp64 gives the reference, fp32 gives "a plain fp32 evaluation of the same formulas", whose distance from the fp64 one is the sensitivity the fp32
bars are 8 x of (BAR32 below).  Nothing here needs a GPU.
"""
import functools

import torch

from oracle import kasf_oracle as O

J = 17
EMBED_NAMES = (("joints_embed", "pos_embed"), ("bone_embed", "bone_pos_embed"), ("limb_embed", "limb_pos_embed"))

# ---- the shapes of the issue (tests/test_gpu_misc.py parametrises over them; the CPU measurement takes the largest of each op)
PROLOGUE_FRAMES = (1, 3, 2047, 2049, 4100)
EMBED_FRAMES = (1, 2, 5, 15, 16, 17, 127, 128, 129, 511, 512, 513, 1031)      # 15 / 16 / 17: those row counts for k_col_finish (nothing else supplies them)
REFUSION_FRAMES = (1, 50, 255, 256, 257, 1000)
GATE_FWD_M = (1, 3, 17, 4099, 65539)
GATE_BWD_M = (1, 3, 17, 2033, 2049, 4099, 12291, 30011)
HEAD_FWD_M = (1, 3, 17, 65539)
HEAD_BWD_M = (1, 17, 2033, 2049, 4099)
REP_BWD_M = (1, 17, 16387)
FINALIZE_NK = ((128, 128), (128, 512))
ADD_N = (128, 128 * 65539)

# ---- the fp32 bars: 8 x the measured sensitivity (max over the op's fp32 outputs, at the op's largest shape, of rel_err(fp32 evaluation, fp64 evaluation)),
# rounded UP to one digit.  Measured values: DESIGN.md 7.2; tests/test_misc_ops_cpu.py::test_fp32_sensitivity_is_within_the_bars re-measures on every run.
BAR32 = {
    "prologue": 2e-6,
    "embed_bwd": 4e-6,
    "refusion_bwd": 4e-5,
    "gate_fwd": 7e-6,
    "gate_bwd": 4e-6,
    "head_fwd": 5e-6,
    "head_bwd": 3e-6,
    "rep_bwd": 6e-7,
    "finalize_ls": 8e-7,
    "add": 7e-7,
}
# No floors: every gradient tensor here -- each of the 204 limb-MLP tensors and the gate's db [3] included -- is judged against ITS OWN largest value.  (They are sums
# over frames / tokens of signed terms, but of random-walk size, not cancelling to rounding level: the fp32 evaluation stays within the bars without a floor.)


def gen(*key):
    return torch.Generator().manual_seed(20261018 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def rel_err(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def fill_params(entries, n_flat):
    """Name-seeded values (oracle.name_seeded_fill) for the prologue's parameters in a flat fp32 array laid out by `entries` (name, offset, shape); the rest 0."""
    want = {n: torch.zeros(s) for n, _, s in entries if n.split(".")[0] in ("bone_refusion", "joints_embed", "bone_embed", "limb_embed") or n.endswith("pos_embed")}
    sd = O.name_seeded_fill(want)
    flat = torch.zeros(n_flat)
    for n, off, s in entries:
        if n in sd:
            flat[off:off + sd[n].numel()] = sd[n].reshape(-1)
    return flat


def named(flat, entries, dtype):
    return {n: flat[off:off + int(torch.tensor(s).prod())].view(s).to(dtype) for n, off, s in entries}


def refusion_module(P, dtype):
    """oracle._BoneRefusion holding the limb-MLP values of P (name -> tensor) in `dtype`"""
    m = O._BoneRefusion().to(dtype)
    m.load_state_dict({n[len("bone_refusion."):]: P[n].to(dtype) for n in P if n.startswith("bone_refusion.")}, strict=True)
    return m


# ------------------------------------------------------------------------------------------------ prologue
@functools.lru_cache(maxsize=None)
def prologue_x(frames):
    """[frames,17,3] fp32: x, y in (-1, 1), confidence in (0, 1); planted: zero-length bones (child == parent), an all-zero frame, and the same again in the frames a
    workgroup reaches on its second walk (2,048 onwards)"""
    g = gen(1, frames)
    x = torch.rand(frames, J, 3, generator=g)
    x[..., :2] = x[..., :2] * 2 - 1
    for f0 in (0, 2048, 4096):
        if f0 < frames:
            x[f0, 2, :2] = x[f0, 3, :2]                 # bone 2 (child 2, parent 3)
            x[f0, 8, :2] = x[f0, 14, :2]                # bone 13 (child 8, parent 14)
        if f0 + 2 < frames:
            x[f0 + 2] = 0.0                             # every bone of the frame has length zero
    return x


def prologue_ref(x, P):
    """x [F,17,3], P name -> tensor, all of one dtype -> bone3, limb3 [F,17,3], xj, xb, xl [F*17,128]"""
    with torch.no_grad():
        bone3 = O.bone_decompose(x[None])[0]
        limb3 = refusion_module(P, x.dtype)(x[None])[0]
        out = {"bone3": bone3, "limb3": limb3}
        for (emb, pos), src, name in zip(EMBED_NAMES, (x, bone3, limb3), ("xj", "xb", "xl")):
            out[name] = (src @ P[emb + ".weight"].T + P[emb + ".bias"] + P[pos][0]).reshape(-1, 128)
    return out


# ------------------------------------------------------------------------------------------------ embedding backward
@functools.lru_cache(maxsize=None)
def embed_inputs(frames):
    g = gen(2, frames)
    return dict(g=torch.randn(frames * J, 128, generator=g), in3=torch.randn(frames * J, 3, generator=g), w=torch.randn(128, 3, generator=g) * 3 ** -0.5)


def embed_bwd_ref(g, in3, w):
    return dict(dw=g.T @ in3, db=g.sum(0), dpos=g.view(-1, J, 128).sum(0), din3=g @ w)


# ------------------------------------------------------------------------------------------------ limb-refusion backward
@functools.lru_cache(maxsize=None)
def refusion_inputs(frames):
    g = gen(3, frames)
    x = torch.rand(frames, J, 3, generator=g)
    x[..., :2] = x[..., :2] * 2 - 1
    return dict(x=x, dlimb3=torch.randn(frames, J, 3, generator=g))


def refusion_bwd_ref(x, dlimb3, P):
    """-> name -> gradient of the 204 limb-MLP tensors (autograd of oracle._BoneRefusion)"""
    m = refusion_module(P, x.dtype)
    m(x[None])[0].backward(dlimb3)
    return {"bone_refusion." + n: p.grad for n, p in m.named_parameters()}


def refusion_err(got, ref):
    """worst per-tensor error of the 204, each against its own largest value -> (error, name)"""
    errs = {n: rel_err(got[n], ref[n]) for n in ref}
    worst = max(errs, key=errs.get)
    return errs[worst], worst


# ------------------------------------------------------------------------------------------------ gate
@functools.lru_cache(maxsize=None)
def gate_inputs(M, scale=1.0):
    g = gen(4, M)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(xa=r(M, 128), xg=r(M, 128), xb=r(M, 128), w=r(3, 384) * 0.05 * scale, bias=1 / 3 + 0.1 * r(3), g=r(M, 128), g1=r(M, 128), g2=r(M, 128))


def gate_fwd_ref(xa, xg, xb, w, bias, adaptive):
    if adaptive:
        alpha = torch.softmax(torch.cat([xa, xg, xb], dim=1) @ w.T + bias, dim=1)
    else:
        alpha = torch.full((xa.shape[0], 3), 1.0 / 3.0, dtype=xa.dtype)
    return dict(alpha=alpha, out=alpha[:, 0:1] * xa + alpha[:, 1:2] * xg + alpha[:, 2:3] * xb)


def gate_bwd_ref(g, xa, xg, xb, w, alpha, adaptive):
    """gradients for g = d/d(out) with alpha [M,3] GIVEN (the stored one: an operand of the kernel): softmax backward written out"""
    xs = (xa, xg, xb)
    if adaptive:
        da = torch.stack([(g * x).sum(1) for x in xs], dim=1)
        dl = alpha * (da - (alpha * da).sum(1, keepdim=True))
        dx = dl @ w                                     # [M,384]
        out = {"dw": dl.T @ torch.cat(xs, dim=1), "db": dl.sum(0), "dl": dl}
    else:
        dx = torch.zeros(g.shape[0], 384, dtype=g.dtype)
        out = {}
    for k, n in enumerate(("ga", "gg", "gb")):
        out[n] = alpha[:, k:k + 1] * g + dx[:, 128 * k:128 * (k + 1)]
    return out


# ------------------------------------------------------------------------------------------------ head
@functools.lru_cache(maxsize=None)
def head_inputs(M):
    g = gen(5, M)
    rep = torch.tanh(torch.randn(M, 512, generator=g))
    rep[0, 0], rep[0, 7], rep[M - 1, 511], rep[M // 2, 130] = 1.0, -1.0, 1.0, -1.0       # saturated tanh: exact in both dtypes
    return dict(rep=rep, w=torch.randn(3, 512, generator=g) * 512 ** -0.5, bias=0.05 * torch.randn(3, generator=g), dy=torch.randn(M, 3, generator=g),
                drep=torch.randn(M, 512, generator=g))


def head_fwd_ref(rep, w, bias):
    return rep @ w.T + bias


def head_bwd_ref(dy, rep, w):
    return dict(dpre=(dy @ w) * (1 - rep * rep), dw=dy.T @ rep, db=dy.sum(0))


def rep_bwd_ref(drep, rep):
    return drep * (1 - rep * rep)


# ------------------------------------------------------------------------------------------------ layer-scale finish, add
@functools.lru_cache(maxsize=None)
def finalize_inputs(N, K):
    g = gen(6, N, K)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(dw=r(N, K), w=r(N, K) * K ** -0.5, bias=0.05 * r(N), ls=0.5 + torch.rand(N, generator=g), db=r(N))


def finalize_ref(dw, w, bias, ls, db):
    return dict(dls=(w * dw).sum(1) + bias * db, dw=dw * ls[:, None], db=db * ls)


@functools.lru_cache(maxsize=None)
def add_inputs(n):
    g = gen(7, n)
    return tuple(torch.randn(n, generator=g) for _ in range(4))


# ------------------------------------------------------------------------------------------------ the CPU measurement behind BAR32
def _sens(fn, ops, keys=None, err=rel_err):
    """max over the outputs of err(fn in fp32, fn in fp64) on the same fp32-representable operands"""
    r64 = fn(*[o.double() if torch.is_tensor(o) else o for o in ops])
    r32 = fn(*[o.float() if torch.is_tensor(o) else o for o in ops])
    return {k: err(r32[k], r64[k]) for k in (keys or r64)}


def measure_fp32_sensitivity(P32):
    """P32: name -> fp32 tensor of the prologue's parameters.  -> op -> {output: rel_err(fp32 evaluation, fp64 evaluation)} at the op's largest listed shape"""
    out = {}
    x = prologue_x(max(PROLOGUE_FRAMES))
    r64 = prologue_ref(x.double(), {n: t.double() for n, t in P32.items()})
    r32 = prologue_ref(x, P32)
    out["prologue"] = {k: rel_err(r32[k], r64[k]) for k in r64}
    i = embed_inputs(max(EMBED_FRAMES))
    out["embed_bwd"] = _sens(embed_bwd_ref, (i["g"], i["in3"], i["w"]))
    i = refusion_inputs(max(REFUSION_FRAMES))
    g64 = refusion_bwd_ref(i["x"].double(), i["dlimb3"].double(), {n: t.double() for n, t in P32.items()})
    g32 = refusion_bwd_ref(i["x"], i["dlimb3"], P32)
    out["refusion_bwd"] = {"worst of 204": refusion_err(g32, g64)[0]}
    i = gate_inputs(max(GATE_FWD_M))
    out["gate_fwd"] = _sens(lambda *a: gate_fwd_ref(*a, 1), (i["xa"], i["xg"], i["xb"], i["w"], i["bias"]))
    i = gate_inputs(max(GATE_BWD_M))
    alpha = gate_fwd_ref(i["xa"], i["xg"], i["xb"], i["w"], i["bias"], 1)["alpha"]       # the fp32 alpha both evaluations are handed, as the kernel is
    out["gate_bwd"] = _sens(lambda g, g1, g2, *a: gate_bwd_ref(g + g1 + g2, *a, 1), (i["g"], i["g1"], i["g2"], i["xa"], i["xg"], i["xb"], i["w"], alpha), keys=("ga", "gg", "gb", "dw", "db"))
    i = head_inputs(max(HEAD_FWD_M))
    out["head_fwd"] = {"out": rel_err(head_fwd_ref(i["rep"], i["w"], i["bias"]), head_fwd_ref(i["rep"].double(), i["w"].double(), i["bias"].double()))}
    i = head_inputs(max(HEAD_BWD_M))
    out["head_bwd"] = _sens(head_bwd_ref, (i["dy"], i["rep"], i["w"]))
    i = head_inputs(max(REP_BWD_M))
    out["rep_bwd"] = {"dpre": rel_err(rep_bwd_ref(i["drep"], i["rep"]), rep_bwd_ref(i["drep"].double(), i["rep"].double()))}
    i = finalize_inputs(128, 512)
    out["finalize_ls"] = _sens(finalize_ref, (i["dw"], i["w"], i["bias"], i["ls"], i["db"]))
    a, b, c, _ = add_inputs(max(ADD_N))
    out["add"] = {"a+b+c": rel_err(a + b + c, a.double() + b.double() + c.double())}
    return out
