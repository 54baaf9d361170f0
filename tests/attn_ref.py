"""Operands and references of tests/test_gpu_attn.py (the attention cores of csrc/k_attn.hip and k_attn_mfma.hip, the fused-d_o backward kernels and the fused
attention-block forward of csrc/k_attn_blk.hip on their own), kept apart from the GPU tests so that the CPU suite can measure what the bars are derived from
(tests/test_attn_ops_cpu.py).  The conventions are those of tests/dense_ref.py.

Every reference is plain torch math on the operands AS THE KERNEL SEES THEM (already rounded to the storage dtype), written once and evaluated
  * in fp64: the reference;
  * in fp32: whose distance from the fp64 one is the sensitivity the fp32 bars are 8 x of (BAR32);
  * in fp64 with a rounding at every point where a kernel holds a 16-bit value (`Rounded`): its distance from the fp64 one is what the bf16 bars are 2 x of (DIST16).
The 16-bit points are listed at each reference.  Nothing here needs a GPU, and no number in the tables below comes from a device run.

Tokens are [batch][frame][joint] (M = B * T * 17 rows).  A GROUP is what one softmax runs over: mode 0 (spatial) the 17 joints of frame G = b * T + t, mode 1
(temporal) the T frames of track G = b * 17 + j; the references work on [G, L, C] views (`to_groups` / `from_groups`).
"""
import functools

import torch

from tests.dense_ref import LN_EPS, PLANT_KINDS, Exact, Rounded, gen, ln, ln_params, row_err, row_excess, stored  # noqa: F401  (re-exported for the tests)

J = 17
F64 = torch.float64

# ---- the shapes of the issue (tests/test_gpu_attn.py parametrises over them)
T_EDGES = (1, 4, 31, 32, 33, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256)
CORE_B = 2
# (heads, mode, B, T): bf16 mode
CORE_BF16 = [(8, 1, CORE_B, T) for T in T_EDGES + (257,)] + [(8, 0, 1, 4), (8, 0, 3, 27)] + [(4, 1, CORE_B, T) for T in T_EDGES] + \
            [(h, 1, CORE_B, T) for h in (2, 16) for T in (27, 96)]
CORE_FP32 = [(h, 1, CORE_B, T) for h in (16, 8, 4, 2) for T in (4, 27, 81)] + [(8, 1, CORE_B, 256), (2, 1, CORE_B, 157)]
CORE_PADDED = [(8, 1, CORE_B, 27), (8, 1, CORE_B, 96), (8, 1, CORE_B, 128), (4, 1, CORE_B, 33), (2, 1, CORE_B, 27)]    # one per kernel family: ld + 8 elements
# fused-d_o backward: name -> [(mode, B, T)]
FUSED_DO = {
    "pers9": [(0, 1, 4), (0, 41, 27), (1, 2, 4), (1, 2, 17)],
    "pers16": [(1, 2, 18), (1, 2, 31), (1, 2, 32), (1, 31, 32)],          # B = 31: 527 groups over 512 workgroups: a second walk and empty workgroups
    "long": [(1, 2, 33), (1, 2, 64), (1, 2, 65), (1, 2, 96)],
    "kt16": [(1, B, T) for T in (33, 64, 82, 96) for B in (1, 3, 16)],
    "kt9": [(1, B, T) for T in (65, 81) for B in (1, 3, 16)],
}
# block forward: name -> [(mode, B, T)] ; flat is listed by frames (B = frames, T = 1: the spatial kernel sees B * T only)
BLOCK = {
    "flat": [(0, f, 1) for f in (1, 2, 3, 32, 1025)],
    "rp": [(1, 1, T) for T in (4, 9, 16, 17, 27, 31, 32)] + [(1, 31, 32), (1, 46, 27)],
    "rp3": [(1, 1, T) for T in (33, 64, 65, 81, 95, 96)] + [(1, 16, 81), (1, 31, 96)],
}
BLOCK_LONG = {0: (0, 24577, 1), 1: (0, 12289, 1)}          # bone -> the 49-frames-per-workgroup case (training mode only)
HANDOVER = [(1, 3, T) for T in (33, 64, 65, 81, 96)] + [(1, 3, 27), (0, 3, 9)]       # rp3 -> kt;  rp -> pers<16>;  flat -> pers<9>

# ---- the bars.  BAR32[op.output]: 8 x the fp32 evaluation's distance from the fp64 one, in the measure the GPU test applies (per (token, head) over the (group, head)
# block's largest |ref|; x_mid per row; lse absolute over max(1, |ref|)), at the op's largest listed shapes with the plants in, rounded UP to one digit.  DIST16: the
# `Rounded` evaluation's distance, same measure.  Measured values: DESIGN.md 7.4; tests/test_attn_ops_cpu.py re-measures on every run.  No BAR32 above 1e-4, no c16 above 3e-2.
BAR32 = {
    "core_fwd.o": 8e-5, "core_fwd.lse": 2e-5,
    "core_bwd.dq": 4e-5, "core_bwd.dk": 5e-5, "core_bwd.dv": 5e-5,
    "fused_do.dq": 4e-5, "fused_do.dk": 4e-5, "fused_do.dv": 7e-5,
    "kt.dq": 2e-5, "kt.dk": 2e-5, "kt.dv": 6e-5,
    "block.q": 3e-5, "block.k": 3e-5, "block.v": 3e-5, "block.o": 5e-5, "block.lse": 2e-6, "block.x_mid": 8e-6,
    # the block backward, stage by stage (measure_bwd: every listed shape, both forms)
    "bwd.xn": 3e-6, "bwd.dq": 8e-6, "bwd.dk": 8e-6, "bwd.dv": 6e-6, "bwd.out": 2e-5, "bwd.dgamma": 4e-6, "bwd.dw": 4e-6, "bwd.dproj": 6e-6, "bwd.dproj_b": 1e-6,
}
# (two digits where one would lift c16 past 3e-2.  lse and x_mid have no 16-bit point in front of them once q | k | v and o are taken as stored: their c is the fp32 bar)
DIST16 = {
    "core_fwd.o": 3e-3, "core_fwd.lse": 0.0,
    "core_bwd.dq": 1.1e-2, "core_bwd.dk": 6e-3, "core_bwd.dv": 6e-3,
    "fused_do.dq": 1.2e-2, "fused_do.dk": 1.1e-2, "fused_do.dv": 9e-3,
    "kt.dq": 1.5e-2, "kt.dk": 1.1e-2, "kt.dv": 8e-3,
    "block.q": 4e-3, "block.k": 4e-3, "block.v": 4e-3, "block.o": 3e-3, "block.lse": 0.0, "block.x_mid": 0.0,
    # (xn and dproj_b = ls1 . colsum(g_mid) have no 16-bit point in front of them)
    "bwd.xn": 0.0, "bwd.dq": 1.4e-2, "bwd.dk": 1.3e-2, "bwd.dv": 1e-2, "bwd.out": 3e-3, "bwd.dgamma": 5e-3, "bwd.dw": 3e-3, "bwd.dproj": 7e-3, "bwd.dproj_b": 0.0,
}


def c16(key):
    return max(BAR32[key], 2 * DIST16[key])


def bar(key, cd):
    return BAR32[key] if cd == "fp32" else c16(key)


# ------------------------------------------------------------------------------------------------ groups
def group_len(T, mode):
    return J if mode == 0 else T


def n_groups(B, T, mode):
    return B * T if mode == 0 else B * J


def to_groups(x, B, T, mode):
    """[M, C] token-major -> [G, L, C]"""
    x = x.reshape(B, T, J, -1)
    return x.reshape(B * T, J, x.shape[-1]) if mode == 0 else x.permute(0, 2, 1, 3).reshape(B * J, T, x.shape[-1])


def from_groups(xg, B, T, mode):
    C = xg.shape[-1]
    return xg.reshape(B * T * J, C) if mode == 0 else xg.reshape(B, J, T, C).permute(0, 2, 1, 3).reshape(B * T * J, C)


def _heads(t, H):
    G, L, _ = t.shape
    return t.reshape(G, L, H, -1).transpose(1, 2)             # [G, H, L, d]


def _merge(t):
    G, H, L, d = t.shape
    return t.transpose(1, 2).reshape(G, L, H * d)


# ------------------------------------------------------------------------------------------------ the launchers' group-to-workgroup arithmetic, restated
def wg_walks(groups, grid):
    """persistent kernels (k_attn_blk_fwd_*, k_attn_bwd_pers): per = ceil(groups / grid), workgroup b owns [b per, min((b + 1) per, groups)) -> (per, [(first, end)] of
    the workgroups that own a group, number of workgroups that own none)"""
    per = (groups + grid - 1) // grid
    owned = [(b * per, min((b + 1) * per, groups)) for b in range(grid) if b * per < groups]
    return per, owned, grid - len(owned)


def block_grid(bone, B, T, mode):
    """kasf_launch_attn_block_fwd at full width (an operator entry never narrows): -> (kernel, grid)"""
    L, groups = group_len(T, mode), n_groups(B, T, mode)
    assert L <= 96
    if L > 32:
        return "rp3", min(groups, 256)
    cap = 256 if bone else 512
    if mode == 0:
        return "flat", min(max((groups + 1) // 2, 1), cap)
    return "rp", min(groups, cap)


def fused_do_grid(B, T, mode, stats):
    """kasf_launch_attn_bwd_fused_do, form 0 -> (kernel, grid, groups the grid has room for)"""
    L, groups = group_len(T, mode), n_groups(B, T, mode)
    if L > 32:
        if stats:
            return ("kt9" if 64 < L <= 81 else "kt16"), 16 * ((groups + 7) // 8), 8 * ((groups + 7) // 8)
        return "long", groups, groups
    return ("pers9" if L <= 17 else "pers16"), min(groups, 512), None


def core_kernel(cd, H, T, mode):
    """the instantiation kasf_launch_attn_fwd / _bwd reach -> (forward, backward)"""
    L = group_len(T, mode)
    if cd == "fp32" or H in (2, 16) or L > 256:
        t = "float" if cd == "fp32" else "bf16"
        return f"k_attn_fwd<{t},{128 // H}>", f"k_attn_bwd<{t},{128 // H}>"
    nkt = 1 if L <= 32 else 3 if L <= 96 else 4 if L <= 128 else 6 if L <= 192 else 8
    if H == 4:
        return f"k_attn_fwd_mfma32<{nkt}>", f"k_attn_bwd_2p32<{nkt}>"
    return f"k_attn_fwd_mfma<{nkt}>", ("k_attn_bwd_mfma<1>" if nkt == 1 else "k_attn_bwd_long<3>" if nkt == 3 else f"k_attn_bwd_2p<{nkt}>")


# ------------------------------------------------------------------------------------------------ the planted heads
PLANTS = ("peaked", "offset", "zeroq", "eqk", "v100")
# peaked: (q x a, k x b): scores of deviation a b at every head dimension.  offset: the SCORE every pair gains, c^2 sqrt(d) for q + c, k + c: 70 is c = 4.2 at d = 16 (the
# issue's + 6 is 144, where the fp32 evaluation of the reference alone is 1.7e-5 from fp64 -- ulp(144) = 1.5e-5 -- and 8 x that passes the 1e-4 cap: softened until it
# fits, 1.2e-5.  Scores past 88.7, where exp overflows fp32, then come from the offset head's upper tail (70 +- 6) and, in most rows of 27 or more keys, from the
# peaked head (deviation 32)); 16 is the issue's mild + 2 at d = 16
# At other head dimensions the offset keeps c^2 d (what the fp32 error of a score grows with) at its d = 16 value: scores of 99 at d = 8, 49 at d = 32 and 35 at d = 64 (no overflow at the last two).
# "soft" is what the kt kernels' backward cases carry: their delta = <o, d_o> comes from the bf16 o, and under the mild plants the `Rounded` reference is 2.1e-2 away.
# Backward cases of groups shorter than 8 positions carry "soft" (a peaked head of 4 keys leaves gradients that are differences of nearly cancelling terms: mild at
# T = 4 puts the fp32 evaluation 5.6e-5 and the `Rounded` one 3.1e-2 away), the kt kernels and the hand-over "faint" (under "soft" the `Rounded` reference is 2.2e-2 away).
LEVELS = {"strong": {"peaked": (8.0, 4.0), "offset": 70.0}, "mild": {"peaked": (4.0, 2.0), "offset": 16.0}, "soft": {"peaked": (2.0, 2.0), "offset": 4.0},
          "faint": {"peaked": (1.25, 1.25), "offset": 1.0}, "none": {"peaked": (1.0, 1.0), "offset": 0.0}}


def fwd_level(L):
    """forward cases: the strong plants at every group length"""
    return "strong"


def bwd_level(L, kt=False):
    """the plant level a backward case carries with all three gradients held"""
    return "faint" if kt else "soft" if L < 8 else "mild"


def offset_of(score, d):
    return (4.0 * score / d) ** 0.5


def plant_heads(H, G):
    """{plant: (head, groups mask [G])}: every plant on a head of its own; with fewer than five heads the plants take turns over the groups (G % rounds)"""
    rounds = (len(PLANTS) + H - 1) // H
    gi = torch.arange(G)
    return {p: (k % H, gi % rounds == k // H) for k, p in enumerate(PLANTS)}


def plant_qkv(qg, kg, vg, H, strong):
    """[G, L, 128] each -> planted copies and the (group, head) blocks whose gradient is analytically zero: {"dq": [G, H] bool (equal keys), "dk": (zero queries)}"""
    qg, kg, vg = qg.clone(), kg.clone(), vg.clone()
    G, d = qg.shape[0], 128 // H
    lv = LEVELS[strong if isinstance(strong, str) else "strong" if strong else "mild"]
    zero = {"dq": torch.zeros(G, H, dtype=torch.bool), "dk": torch.zeros(G, H, dtype=torch.bool)}
    for p, (h, m) in plant_heads(H, G).items():
        c = slice(h * d, (h + 1) * d)
        if p == "peaked":
            qg[m, :, c] *= lv[p][0]
            kg[m, :, c] *= lv[p][1]
        elif p == "offset":
            qg[m, :, c] += offset_of(lv[p], d)
            kg[m, :, c] += offset_of(lv[p], d)
        elif p == "zeroq":
            qg[m, :, c] = 0.0
            zero["dk"][m, h] = True
        elif p == "eqk":
            kg[m, :, c] = kg[m, :1, c]
            zero["dq"][m, h] = True
        else:
            vg[m, :, c] *= 100.0
    return qg, kg, vg, zero


# ------------------------------------------------------------------------------------------------ measures
def head_err(got, ref, H, zero=None, excess=False):
    """grouped [G, L, 128]: per (token, head) the largest error of the head's slice over the largest |ref| of the (group, head) block (where `zero` [G, H] marks a block
    of the reference as analytically zero: over the group's largest |ref| of all heads); excess: per element minus the output's own bf16 ulp 2^-8 |ref|.
    -> (worst, (group, position, head))"""
    got, ref = got.detach().double(), ref.detach().double()
    G, L, _ = ref.shape
    d = (got - ref).abs()
    if excess:
        d = d - 2.0 ** -8 * ref.abs()
    e = d.reshape(G, L, H, -1).amax(-1)
    den = ref.abs().reshape(G, L, H, -1).amax((1, 3))
    if zero is not None:
        den = torch.where(zero, ref.abs().reshape(G, -1).amax(1, keepdim=True).expand(G, H), den)
    e = e / den.clamp_min(1e-300)[:, None, :]
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    k = int(e.argmax())
    return float(e.reshape(-1)[k]), (k // (L * H), k // H % L, k % H)


def lse_err(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    e = (got - ref).abs() / ref.abs().clamp_min(1.0)
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    return float(e.max())


# ------------------------------------------------------------------------------------------------ the cores
def _scores(qg, kg, H):
    return (_heads(qg, H) @ _heads(kg, H).transpose(-1, -2)) * (128 // H) ** -0.5


def core_fwd(qg, kg, vg, H, R=Exact):
    """o = softmax(q k^T / sqrt(d)) v per (group, head); lse [G, L, H] = log sum_j exp(s_ij).
    16-bit points (bf16 MFMA cores): the UNNORMALISED exponentials exp(s - max) are the bf16 operand of the P V product, the division by their fp32 sum follows;
    o's own rounding is the output's ulp."""
    s = _scores(qg, kg, H)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    z = e.sum(-1, keepdim=True)
    return dict(o=_merge((R.bf(e) @ _heads(vg, H)) / z), lse=(mx + torch.log(z)).squeeze(-1).transpose(1, 2))


def core_bwd(qg, kg, vg, dog, H, R=Exact, o_saved=None, lse=None):
    """Backward of core_fwd for the upstream gradient d_o, written out (held to autograd by tests/test_attn_ops_cpu.py):
         P = softmax(s), dP = d_o v^T, delta = rowsum(P dP) = <o, d_o>, dS = P (dP - delta) / sqrt(d);  dq = dS k, dk = dS^T q, dv = P^T d_o.
    16-bit points: P and dS as bf16 MFMA operands; dq, dk, dv's own roundings are the outputs' ulps.
    k_attn_bwd_kt (o_saved, lse given): P is rebuilt as exp(s - lse) and delta = <o_saved, d_o> from the forward's stored (bf16) output."""
    s = _scores(qg, kg, H)
    qh, kh, vh, doh = _heads(qg, H), _heads(kg, H), _heads(vg, H), _heads(dog, H)
    P = torch.softmax(s, -1) if lse is None else torch.exp(s - lse.transpose(1, 2).unsqueeze(-1))
    dP = doh @ vh.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True) if o_saved is None else (_heads(o_saved, H) * doh).sum(-1, keepdim=True)
    dS = R.bf(P * (dP - delta) * (128 // H) ** -0.5)
    return dict(dq=_merge(dS @ kh), dk=_merge(dS.transpose(-1, -2) @ qh), dv=_merge(R.bf(P).transpose(-1, -2) @ doh))


@functools.lru_cache(maxsize=4)
def core_inputs(H, mode, B, T, strong):
    """q, k, v, d_o [M, 128] token-major (fp32 values) with the planted heads in, and the zero-block masks"""
    g = gen(21, H, mode, B, T, len(str(strong)))
    M = B * T * J
    r = lambda *s: torch.randn(*s, generator=g)
    qg, kg, vg, zero = plant_qkv(*(to_groups(r(M, 128), B, T, mode) for _ in range(3)), H, strong)
    return dict(q=from_groups(qg, B, T, mode), k=from_groups(kg, B, T, mode), v=from_groups(vg, B, T, mode), d_o=r(M, 128), zero=zero, _model=("q", "k", "v", "d_o"))


def core_eval(i, H, mode, B, T, dtype=F64, R=Exact):
    """forward and backward of one case on the stored operands `i` -> grouped outputs"""
    qg, kg, vg, dog = (to_groups(i[n].to(dtype), B, T, mode) for n in ("q", "k", "v", "d_o"))
    return {**core_fwd(qg, kg, vg, H, R), **core_bwd(qg, kg, vg, dog, H, R)}


# ------------------------------------------------------------------------------------------------ fused-d_o backward
@functools.lru_cache(maxsize=4)
def fused_inputs(mode, B, T, strong=False):
    g = gen(22, mode, B, T, len(str(strong)))
    M = B * T * J
    r = lambda *s: torch.randn(*s, generator=g)
    qg, kg, vg, zero = plant_qkv(*(to_groups(r(M, 128), B, T, mode) for _ in range(3)), 8, strong)
    W, ls1 = r(128, 128) * 128 ** -0.5, 0.5 + torch.rand(128, generator=g)
    return dict(q=from_groups(qg, B, T, mode), k=from_groups(kg, B, T, mode), v=from_groups(vg, B, T, mode), g_mid=r(M, 128), wts=(ls1[:, None] * W).T.contiguous(),
                zero=zero, _model=("q", "k", "v", "g_mid", "wts"))           # wts [c][n] = ls1[n] W[n][c]: the packed operand wproj_t_scaled


def fused_eval(i, mode, B, T, dtype=F64, R=Exact, stats=None):
    """16-bit points on top of core_bwd's: d_o = bf16(g_mid wts^T).  stats = (o [G, L, 128], lse [G, L, 8]): the kt kernels' operands."""
    qg, kg, vg = (to_groups(i[n].to(dtype), B, T, mode) for n in ("q", "k", "v"))
    dog = to_groups(R.bf(i["g_mid"].to(dtype) @ i["wts"].to(dtype).T), B, T, mode)
    o, lse = (None, None) if stats is None else (stats[0].to(dtype), stats[1].to(dtype))
    return core_bwd(qg, kg, vg, dog, 8, R, o, lse)


def handover_zero(B, T, mode):
    """the blocks of the hand-over's gradients that the block forward's planted weight rows make zero: zero keys on head 4 (dq), zero queries on head 3 (dk)"""
    zero = {n: torch.zeros(n_groups(B, T, mode), 8, dtype=torch.bool) for n in ("dq", "dk")}
    zero["dq"][:, 4] = zero["dk"][:, 3] = True
    return zero


def kt_stats(i, mode, B, T, rounded=True):
    """what the training forward leaves for k_attn_bwd_kt, from the fp64 reference on the stored operands: o rounded to bf16, lse to fp32 (grouped)"""
    f = core_fwd(*(to_groups(i[n].to(F64), B, T, mode) for n in ("q", "k", "v")), 8)
    return (f["o"].to(torch.bfloat16).to(F64), f["lse"].float().to(F64)) if rounded else (f["o"], f["lse"])


# ------------------------------------------------------------------------------------------------ block forward
def plant_rows(x, rows, g):
    """the LayerNorm plants of dense_ref.plant on the given token rows, one kind per row in PLANT_KINDS order -> {kind: [rows]}"""
    where = {k: [] for k in PLANT_KINDS}
    for n, row in enumerate(rows):
        kind = PLANT_KINDS[n % len(PLANT_KINDS)]
        r = torch.randn(128, generator=g)
        x[row] = {"const": torch.full((128,), 0.75), "zero": torch.zeros(128), "tiny": 1e-3 * r, "mean32": 32 + r, "big": 1e3 * r}[kind]
        where[kind].append(row)
    return where


def token_of(G, i, T, mode):
    return G * J + i if mode == 0 else (G // J) * T * J + i * J + G % J


def planted_groups(bone, B, T, mode):
    """first group, last group, and the second group of workgroup 0's walk (group 1 where a workgroup owns more than one, else none)"""
    groups = n_groups(B, T, mode)
    per = wg_walks(groups, block_grid(bone, B, T, mode)[1])[0]
    return sorted({0, groups - 1} | ({1} if per > 1 else set()))


@functools.lru_cache(maxsize=2)
def block_inputs(bone, mode, B, T, level="strong"):
    """level: the planted heads' strength (LEVELS); the hand-over cases, whose q | k | v feed a backward kernel, carry the soft ones"""
    lv = LEVELS[level]
    g = gen(23, bone, mode, B, T, len(level))
    M, L = B * T * J, group_len(T, mode)
    r = lambda *s: torch.randn(*s, generator=g)
    x, xl = r(M, 128), r(M, 128)
    last = n_groups(B, T, mode) - 1                          # (the last group carries its plants on its last positions: the very last token is a constant row)
    rows = [token_of(G, L - 1 - p if G == last and G > 0 else p, T, mode) for G in planted_groups(bone, B, T, mode) for p in range(min(5, L))]
    where = plant_rows(x, rows, g)
    where_l = plant_rows(xl, rows[::-1], g)                  # (the limb stream carries the kinds in the opposite order: a constant x row meets a big x_limb row)
    ln_g, ln_b = ln_params(g)
    lnl_g, lnl_b = ln_params(g)
    wq, wkv = r(128 if bone else 384, 128) * 128 ** -0.5, r(256, 128) * 128 ** -0.5
    qr = lambda h: slice(16 * h, 16 * h + 16)
    kw, ko, vo = (wkv, 0, 128) if bone else (wq, 128, 256)   # where the k and v rows of head h live
    kr, vr = (lambda h: slice(ko + 16 * h, ko + 16 * h + 16)), (lambda h: slice(vo + 16 * h, vo + 16 * h + 16))
    kb = lnl_b if bone else ln_b
    wq[qr(1)] *= lv["peaked"][0]                             # head 1 peaked: q x 8, k x 4
    kw[kr(1)] *= lv["peaked"][1]
    c = offset_of(lv["offset"] * (1.5 if level == "strong" else 1.0), 16)     # head 2 offset: the LayerNorm's beta carries a constant through the weight rows: q + c, k + c (strong: c = 6)
    wq[qr(2)] += c * ln_b / (ln_b @ ln_b)
    kw[kr(2)] += c * kb / (kb @ kb)
    wq[qr(3)] = 0.0                                          # head 3: zero queries
    kw[kr(4)] = 0.0                                          # head 4: equal (zero) keys
    kw[vr(5)] *= 100.0                                       # head 5: v x 100
    return dict(x=x, xl=xl if bone else None, ln_g=ln_g, ln_b=ln_b, lnl_g=lnl_g if bone else None, lnl_b=lnl_b if bone else None, wq=wq, wkv=wkv if bone else None,
                wproj=r(128, 128) * 128 ** -0.5, bproj=0.5 * r(128), ls1=0.5 + torch.rand(128, generator=g), where=where, where_l=where_l,
                _model=("x", "xl", "wq", "wkv", "wproj"))


def block_ref(i, B, T, mode, dtype=F64, R=Exact, chunk=2048, given=None):
    """x_mid = x + ls1 (proj(attention(q, k, v)) + bproj), q | k | v = LN(x) Wqkv^T (bone: q = LN(x) Wq^T, k | v = LN_limb(x_limb) Wkv^T), 8 heads.
    16-bit points: LN(x) (LN_limb(x_limb)) as the GEMM operand; q | k | v as stored and as the cores' operands; core_fwd's P; the heads' outputs o as stored and as the
    projection's operand; x_mid's own rounding is the output's ulp.  -> token-major q, k, v, o, x_mid [M, 128] and lse [M, 8]
    given: {"q", "k", "v"} and / or {"o"} [M, 128] as a device stored them: o and lse are then the core's on the given q | k | v, x_mid the projection's on the given o
    (q, k, v and o are returned as computed from x and from the core all the same).  The GPU test holds o and lse to the
    core on the STORED q | k | v, and x_mid to the projection of the STORED o: end to end, the bf16 rounding of q and k alone moves a peaked head's one-hot softmax
    to another key, and the reference itself is 1.0 from its `Rounded` evaluation.
    Spatial cases of more than `chunk` frames are evaluated `chunk` frames at a time (frames are independent)."""
    given = given or {}
    if mode == 0 and B * T > chunk:
        parts = []
        for f0 in range(0, B * T, chunk):
            f1 = min(f0 + chunk, B * T)
            sub = {k: (v[f0 * J:f1 * J] if k in ("x", "xl") and v is not None else v) for k, v in i.items()}
            parts.append(block_ref(sub, f1 - f0, 1, 0, dtype, R, chunk, {k: v[f0 * J:f1 * J] for k, v in given.items()}))
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    c = lambda n: i[n].to(dtype) if i[n] is not None else None
    x = c("x")
    xn = R.bf(ln(x, c("ln_g"), c("ln_b")))
    if i["xl"] is None:
        q, k, v = R.bf(xn @ c("wq").T).split(128, dim=1)
    else:
        q = R.bf(xn @ c("wq").T)
        k, v = R.bf(R.bf(ln(c("xl"), c("lnl_g"), c("lnl_b"))) @ c("wkv").T).split(128, dim=1)
    f = core_fwd(*(to_groups(given[n].to(dtype) if n in given else t, B, T, mode) for n, t in (("q", q), ("k", k), ("v", v))), 8, R)
    o = R.bf(from_groups(f["o"], B, T, mode))
    return dict(q=q, k=k, v=v, o=o, lse=from_groups(f["lse"], B, T, mode),
                x_mid=x + c("ls1") * ((given["o"].to(dtype) if "o" in given else o) @ c("wproj").T + c("bproj")))


# ------------------------------------------------------------------------------------------------ block backward (k_attn_bwd_f.hip through kasf_op_attn_block_bwd)
def block_bwd_grid(B, T, mode):
    """kasf_launch_attn_block_bwd at full width: -> (grid, groups per workgroup, workgroups that own a group: the sink's rows and the proj job's tiles)"""
    groups = n_groups(B, T, mode)
    grid = min(groups, 256)
    per = (groups + grid - 1) // grid
    return grid, per, (groups + per - 1) // per


def bwd_planted_groups(B, T, mode):
    """first group, last group, and the second group of workgroup 0's walk"""
    groups = n_groups(B, T, mode)
    return sorted({0, groups - 1} | ({1} if block_bwd_grid(B, T, mode)[1] > 1 else set()))


@functools.lru_cache(maxsize=2)
def block_bwd_inputs(bone, mode, B, T):
    """The operands of the block backward.  No peaked or offset head (as the hand-over cases): zero-query head 3, zero-key head 4, v x 100 head 5; the q and k weight
    rows carry a score scale of 0.5 (with unit-variance q and k the `Rounded` dq | dk | dv alone are 1.7e-2 / 1.8e-2 / 1.3e-2 from fp64: 2 x that is past the 3e-2
    cap).  LayerNorm plants as block_inputs; groups shorter than 8 positions carry two planted rows (constant, zero) instead of five: four planted rows of four give
    equal keys and nearly cancelling terms (dk 6.9e-2 away)."""
    g = gen(24, bone, mode, B, T)
    M, L = B * T * J, group_len(T, mode)
    r = lambda *s: torch.randn(*s, generator=g)
    x, xl = r(M, 128), r(M, 128)
    last = n_groups(B, T, mode) - 1
    n_plants = min(5, L) if L >= 8 else min(2, L)
    rows = [token_of(G, L - 1 - p if G == last and G > 0 else p, T, mode) for G in bwd_planted_groups(B, T, mode) for p in range(n_plants)]
    where = plant_rows(x, rows, g)
    where_l = plant_rows(xl, rows[::-1], g)
    ln_g, ln_b = ln_params(g)
    lnl_g, lnl_b = ln_params(g)
    wq, wkv = r(128 if bone else 384, 128) * 128 ** -0.5, r(256, 128) * 128 ** -0.5
    kw, ko, vo = (wkv, 0, 128) if bone else (wq, 128, 256)
    wq[:128] *= 0.5 ** 0.5                                   # q and k share the score scale of 0.5
    kw[ko:ko + 128] *= 0.5 ** 0.5
    wq[16 * 3:16 * 4] = 0.0
    kw[ko + 16 * 4:ko + 16 * 5] = 0.0
    kw[vo + 16 * 5:vo + 16 * 6] *= 100.0
    proj_w, ls1 = r(128, 128) * 128 ** -0.5, 0.5 + torch.rand(128, generator=g)
    return dict(x=x, xl=xl if bone else None, ln_g=ln_g, ln_b=ln_b, lnl_g=lnl_g if bone else None, lnl_b=lnl_b if bone else None, wq=wq, wkv=wkv if bone else None,
                proj_w=proj_w, proj_b=0.5 * r(128), ls1=ls1, wts=(ls1[:, None] * proj_w).T.contiguous(), g_mid=r(M, 128), outl0=r(M, 128) if bone else None,
                where=where, where_l=where_l, _model=("x", "xl", "wq", "wkv", "wts", "g_mid", "outl0"))


def block_bwd_ref(i, B, T, mode, dtype=F64, R=Exact, given=None):
    """Every output of kasf_op_attn_block_bwd, stage by stage.  16-bit points: LN(x) (LN_limb(x_limb)) as stored and as operand; q | k | v and d_o = g_mid wts^T as
    the core's operands; core_bwd's P and dS; dq | dk | dv as stored and as operands; the data gradient's staging tile bf16(dq | dk | dv . W) in front of the LayerNorm
    backward; one bf16 tile per token split of the streaming weight gradient (dense_ref.jobs_splits); o = bf16(P v) as the proj gradient's operand and one bf16 tile
    of G = g_mid^T o per workgroup (block_bwd_grid).  given: {"xn", "xnl"} and / or {"dq", "dk", "dv"} [M, 128] as a device stored them: the later stages then run
    on those (the earlier outputs are returned as computed all the same)."""
    from tests.dense_ref import jobs_splits, ln_bwd, ls_algebra
    given = given or {}
    c = lambda n: i[n].to(dtype) if i.get(n) is not None else None
    take = lambda n, t: given[n].to(dtype) if n in given else R.bf(t)
    bone = i["xl"] is not None
    x, g, wq, wkv = c("x"), c("g_mid"), c("wq"), c("wkv")
    out = dict(xn=ln(x, c("ln_g"), c("ln_b")))
    xn = take("xn", out["xn"])
    if bone:
        out["xnl"] = ln(c("xl"), c("lnl_g"), c("lnl_b"))
        xnl = take("xnl", out["xnl"])
        q, (k, v) = R.bf(xn @ wq.T), R.bf(xnl @ wkv.T).split(128, dim=1)
    else:
        q, k, v = R.bf(xn @ wq.T).split(128, dim=1)
    qg, kg, vg, dog = (to_groups(t, B, T, mode) for t in (q, k, v, R.bf(g @ c("wts").T)))
    gr = core_bwd(qg, kg, vg, dog, 8, R)
    for n in ("dq", "dk", "dv"):
        out[n] = from_groups(gr[n], B, T, mode)
    dq, dk, dv = (take(n, out[n]) for n in ("dq", "dk", "dv"))
    if bone:
        dxn, dkv = R.bf(dq @ wq), torch.cat([dk, dv], 1)
        dxl, out["dgamma_l"], out["dbeta_l"] = ln_bwd(R.bf(dkv @ wkv), c("xl"), c("lnl_g"))
        out["out_limb"] = c("outl0") + dxl
    else:
        dxn = R.bf(torch.cat([dq, dk, dv], 1) @ wq)
    dx, out["dgamma"], out["dbeta"] = ln_bwd(dxn, x, c("ln_g"))
    out["out"] = g + dx
    splits, sl = jobs_splits(x.shape[0], (128, 256) if bone else (384,))
    tn = lambda A, Bm: sum(R.bf(A[z * sl:(z + 1) * sl].T @ Bm[z * sl:(z + 1) * sl]) for z in range(splits)) if R.rounded else A.T @ Bm
    if bone:
        out["dw_mix"], out["dw_kv"] = tn(dq, xn), tn(dkv, xnl)
    else:
        out["dw_mix"] = tn(torch.cat([dq, dk, dv], 1), xn)
    og = R.bf(_merge(R.bf(torch.softmax(_scores(qg, kg, 8), -1)) @ _heads(vg, 8)))
    gg = to_groups(g, B, T, mode)
    _, per, active = block_bwd_grid(B, T, mode)
    tile = lambda a, b: torch.einsum("glk,glc->kc", a, b)
    Gm = sum(R.bf(tile(gg[w * per:(w + 1) * per], og[w * per:(w + 1) * per])) for w in range(active)) if R.rounded else tile(gg, og)
    out["dproj_w"], out["dproj_b"], out["dls1"] = ls_algebra(Gm, g.sum(0), c("proj_w"), c("proj_b"), c("ls1"))
    return out


# block backward: name -> [(mode, B, T)]; spatial is listed by frames (257 frames: per = 2, 129 active workgroups and 127 that return at once; 513: per = 3);
# 272 and 527 temporal groups: the second and third walk, a short last range and empty workgroups
BLOCK_BWD = {
    "spatial": [(0, f, 1) for f in (1, 2, 255, 256, 257, 513)],
    "t9": [(1, 1, T) for T in (4, 9, 16, 17)] + [(1, 16, 17)],
    "t16": [(1, 1, T) for T in (18, 27, 31, 32)] + [(1, 16, 27), (1, 31, 32)],
}
BWD_STAGES = {"xn": ("xn", "xnl"), "dq": ("dq",), "dk": ("dk",), "dv": ("dv",), "out": ("out", "out_limb"), "dgamma": ("dgamma", "dbeta", "dgamma_l", "dbeta_l"),
              "dw": ("dw_mix", "dw_kv"), "dproj": ("dproj_w", "dls1"), "dproj_b": ("dproj_b",)}
BWD_STAGE_PASS = {"xn": 0, "dq": 1, "dk": 1, "dv": 1}          # the pass in which a stage is judged: 0 from x, 1 on the stored LN(x), 2 on the stored LN(x) and dq | dk | dv
MEASURE_BWD = sorted({c for cases in BLOCK_BWD.values() for c in cases})          # every listed shape: the whole measurement takes 15 s


def bwd_errs(a, b, B, T, mode, excess):
    """{output: distance} of two evaluations in the measures of the GPU test: dq | dk | dv per (token, head), the token-major outputs per row (`excess`: over the
    stored output's own bf16 ulp), the reductions per tensor"""
    from tests.dense_ref import rel_err
    z = handover_zero(B, T, mode)
    out = {}
    for n in b:
        if n in ("dq", "dk", "dv"):
            out[n] = head_err(to_groups(a[n], B, T, mode), to_groups(b[n], B, T, mode), 8, z.get(n), excess=excess)[0]
        elif n in ("xn", "xnl", "out", "out_limb"):
            out[n] = (row_excess if excess else row_err)(a[n], b[n])[0]
        else:
            out[n] = rel_err(a[n], b[n])
    return out


def measure_bwd(which):
    """bwd.<stage> -> the worst distance over MEASURE_BWD and both forms, each stage on what the stage before stored (the `Rounded` evaluation's values in bf16)"""
    f32 = which == "fp32"
    lo, R = (torch.float32, Exact) if f32 else (F64, Rounded)
    out = {}
    for mode, B, T in MEASURE_BWD:
        for bone in (0, 1):
            i = stored(block_bwd_inputs(bone, mode, B, T), "bf16")
            st = {}
            for k, names in enumerate((("xn", "xnl"), ("dq", "dk", "dv"), ())):
                a, b = block_bwd_ref(i, B, T, mode, lo, R, st), block_bwd_ref(i, B, T, mode, given=st)
                e = bwd_errs(a, b, B, T, mode, excess=not f32)
                for stage, outs in BWD_STAGES.items():
                    if BWD_STAGE_PASS.get(stage, 2) == k:
                        for n in outs:
                            if n in e:
                                out[f"bwd.{stage}"] = max(out.get(f"bwd.{stage}", 0.0), e[n])
                dev = a if not f32 else block_bwd_ref(i, B, T, mode, F64, Rounded, st)
                st = dict(st, **{n: dev[n].to(torch.bfloat16).to(F64) for n in names if n in dev})
    return out


# ------------------------------------------------------------------------------------------------ the CPU measurements behind BAR32 and DIST16
# the largest listed shapes, and the shortest groups (few keys: the least averaging)
MEASURE_CORE = {"fp32": [(8, 1, CORE_B, 256), (2, 1, CORE_B, 157), (16, 1, CORE_B, 81), (4, 1, CORE_B, 81), (8, 1, CORE_B, 4), (16, 1, CORE_B, 4), (4, 1, CORE_B, 4), (2, 1, CORE_B, 4)],
                "bf16": [(8, 1, CORE_B, 257), (8, 0, 3, 27), (8, 0, 1, 4), (8, 1, CORE_B, 4), (4, 1, CORE_B, 256), (4, 1, CORE_B, 4), (2, 1, CORE_B, 96), (16, 1, CORE_B, 96),
                         (16, 1, CORE_B, 27)]}
MEASURE_FUSED = sorted({c for name, cases in FUSED_DO.items() for c in cases})
MEASURE_BLOCK = [(0, 1025, 1), (1, 46, 27), (1, 31, 96)]


def measure(which):
    """which = 'fp32': key -> distance(fp32 evaluation, fp64 evaluation) on fp32 operands; 'bf16': key -> distance(`Rounded` fp64 evaluation, fp64 evaluation) on the
    operands as bf16 mode stores them (without the outputs' own ulp: the GPU test takes that off as well).  Forward outputs carry the strong plants, dq / dk the
    mild ones, dv both.  The worst over the listed shapes of each op."""
    f32 = which == "fp32"
    cd = "fp32" if f32 else "bf16"
    lo, R = (torch.float32, Exact) if f32 else (F64, Rounded)
    out = {}

    def worst(key, v):
        out[key] = max(out.get(key, 0.0), v)

    def grads(op, a, b, H, zero, only_dv):
        for n in ("dv",) if only_dv else ("dq", "dk", "dv"):
            worst(f"{op}.{n}", head_err(a[n], b[n], H, zero.get(n))[0])

    for H, mode, B, T in MEASURE_CORE[cd]:
        for level in (fwd_level(group_len(T, mode)), bwd_level(group_len(T, mode))):
            i = stored(core_inputs(H, mode, B, T, level), cd)
            a, b = core_eval(i, H, mode, B, T, lo, R), core_eval(i, H, mode, B, T)
            if level == fwd_level(group_len(T, mode)):
                worst("core_fwd.o", head_err(a["o"], b["o"], H)[0])
                worst("core_fwd.lse", lse_err(a["lse"], b["lse"]))
            grads("core_bwd", a, b, H, i["zero"], level != bwd_level(group_len(T, mode)))
    for mode, B, T in MEASURE_FUSED:
        L = group_len(T, mode)
        for level in ("strong", bwd_level(L)):
            i = stored(fused_inputs(mode, B, T, level), cd)
            grads("fused_do", fused_eval(i, mode, B, T, lo, R), fused_eval(i, mode, B, T), 8, i["zero"], level == "strong")
        if L > 32:                                          # the kt kernels' form: P from lse, delta from the stored o
            for level in ("mild", "faint"):                 # (strong: exp(s - lse) at s = 96 puts the fp32 evaluation of dv 2.3e-5 away, 8 x that is past the cap)
                i = stored(fused_inputs(mode, B, T, level), cd)
                grads("kt", fused_eval(i, mode, B, T, lo, R, kt_stats(i, mode, B, T, rounded=not f32)), fused_eval(i, mode, B, T), 8, i["zero"], level == "mild")
    for mode, B, T in HANDOVER:                             # the hand-over: the backward on the q | k | v that the block forward stores
        for bone in (0, 1):
            f = block_ref(stored(block_inputs(bone, mode, B, T, "none"), "bf16"), B, T, mode, F64, Rounded)
            i = dict(stored(fused_inputs(mode, B, T, "faint"), cd), **{n: f[n] for n in ("q", "k", "v")})
            kt = group_len(T, mode) > 32
            st = kt_stats(i, mode, B, T, rounded=not f32) if kt else None
            grads("kt" if kt else "fused_do", fused_eval(i, mode, B, T, lo, R, st), fused_eval(i, mode, B, T), 8, handover_zero(B, T, mode), False)
    for mode, B, T in MEASURE_BLOCK:
        for bone in (0, 1):
            i = stored(block_inputs(bone, mode, B, T), cd)
            a, b = block_ref(i, B, T, mode, lo, R), block_ref(i, B, T, mode)
            he = lambda n, a, b: head_err(to_groups(a[n], B, T, mode), to_groups(b[n], B, T, mode), 8, excess=not f32)[0]       # (`Rounded` stores them in bf16)
            for n in ("q", "k", "v"):
                worst(f"block.{n}", he(n, a, b))
            st = {n: a[n].to(torch.bfloat16).to(F64) for n in ("q", "k", "v")}              # stage 2: the core on what a device stored
            a, b = block_ref(i, B, T, mode, lo, R, given=st), block_ref(i, B, T, mode, given=st)
            worst("block.o", he("o", a, b))
            worst("block.lse", lse_err(a["lse"], b["lse"]))
            st["o"] = a["o"].to(torch.bfloat16).to(F64)                                    # stage 3: the projection and the residual on the stored o
            a, b = block_ref(i, B, T, mode, lo, R, given=st), block_ref(i, B, T, mode, given=st)
            worst("block.x_mid", row_err(a["x_mid"], b["x_mid"])[0])
    out.update(measure_bwd(which))
    return out
