"""Operands and references of tests/test_gpu_dense.py (the linear, data-gradient, weight-gradient and MLP kernels of csrc/k_gemm.hip, k_gemm2.hip, k_mlp.hip,
k_mlp2.hip and k_mlp3.hip on their own), kept apart from the GPU tests so that the CPU suite can measure what the bars are derived from
(tests/test_dense_ops_cpu.py).  The conventions are those of tests/misc_ref.py.

Every reference is plain torch math on the operands AS THE KERNEL SEES THEM (already rounded to the storage dtype), written once and evaluated
  * in fp64: the reference;
  * in fp32: "a plain fp32 evaluation of the same formulas", whose distance from the fp64 one is the sensitivity the fp32 bars are 8 x of (BAR32);
  * in fp64 with a rounding at every point where the interface or a kernel's layout stores a 16-bit value (`Rounded`): its distance from the fp64 one is what the
    bf16 bars are 2 x of (DIST16, C16).  The points per op are listed at each reference and in DESIGN.md 7.3.
Nothing here needs a GPU, and no number in the tables below comes from a device run.
"""
import functools
import math

import torch

LN_EPS = 1e-5

# ---- the shapes of the issue (tests/test_gpu_dense.py parametrises over them; the CPU measurement takes the largest of each op)
LINEAR_CASES = ((1, 128, 0), (1, 256, 0), (1, 384, 0), (0, 128, 0), (0, 256, 0), (0, 384, 0), (1, 512, 1), (0, 512, 1))      # (LN, N, act)
LINEAR_M = (1, 31, 32, 33, 63, 64, 65, 8192, 8193, 24577)
# (Kd, dxn_add, resid, accumulate, xn_out): tests/test_gpu_ops.py's DGRAD_CASES
DGRAD_CASES = ((384, False, True, False, True), (128, False, True, False, True), (256, False, False, True, True), (256, True, True, False, False),
               (512, True, True, False, False), (128, True, False, True, False))
DGRAD_M = (1, 32, 33, 64, 65, 8193, 16417, 24577)
# the five combinations kasf_dgrad_wg_supported accepts: name -> (Kd, resid, accumulate, dxn_add + dbias, proj)
WG_FORMS = {"qkv": (384, True, False, False, False), "q": (128, True, False, False, False), "kv": (256, False, True, False, False),
            "uv_bias": (256, True, False, True, False), "q_proj": (128, True, False, False, True)}
DGRAD_WG_M = (1, 33, 8193, 24577, 40003)
WGRAD_NK = ((128, 128), (256, 128), (384, 128), (512, 128), (128, 512))
WGRAD_M = (1, 127, 128, 129, 31743, 31745)
# kasf_op_wgrad_jobs: name -> (N per job, fin job, elements of each reduction, ext job).  att2 / att1_red (the qkv gradient riding in the data-gradient launch) / bone3 are
# the launches of a self-attention / bone block below and above 40,000 tokens, ext_self / ext_bone those behind the fused attention-block backward; one_red2 is a call the
# launcher permits and the engine does not make.
JOBS_MIXES = {"att2": ((128, 384), 0, (), False), "att1_red": ((128,), 0, (384 * 128,), False), "bone3": ((128, 128, 256), 0, (), False),
              "ext_self": ((384,), -1, (), True), "ext_bone": ((128, 256), -1, (), True), "one_red2": ((512,), -1, (128 * 128, 256 * 128), False)}
# Every mix runs the common table (below 248 / tiles x 128 tokens a split is one 128-row tile, so splits = ceil(M / 128): 1 | 1 | 2 | 7 | 16 | 17 | 32 | 33 | 49 splits; 129,
# 769, 2049, 4097: a last split of one row; 6209: a last split of 65 rows, one ring tile and a one-row tail; 128: no tail) and one shape of its own whose splits
# are longer than two ring tiles (the ring reuses a stage): tests/test_dense_ops_cpu.py::test_jobs_tables_meet_the_conditions holds the tables to jobs_splits.
_JOBS_M = (1, 128, 129, 769, 2048, 2049, 4096, 4097, 6209)
JOBS_M = {"att2": _JOBS_M + (24577,), "att1_red": _JOBS_M + (31745,), "bone3": _JOBS_M + (7937,), "ext_self": _JOBS_M + (10625,), "ext_bone": _JOBS_M + (10625,),
          "one_red2": _JOBS_M + (7937,)}
# partial tiles of the reductions / the ext job: case k of a mix's table takes entry k mod len (one_red2's second reduction: 33 parts)
JOBS_PARTS = {"att2": (0,), "bone3": (0,), "att1_red": (1, 17, 256), "ext_self": (1, 16, 17, 33, 256), "ext_bone": (1, 16, 17, 33, 256), "one_red2": (2, 49, 32)}
MLP_FWD_M = {"fp32": (1, 63, 64, 65, 459), "bf16": (1, 31, 32, 33, 8192, 8193, 32769)}
MLP_BWD_M = (1, 31, 32, 33, 64, 65, 4099)
MLP_FUSED_M = (1, 31, 32, 33, 2048, 2049, 10273)
# kasf_op_mlp_bwd_fused_fc2 (tests/test_gpu_sink_forms.py): 16,417 tokens are 514 tiles of 32, so k_lnbwd_sum4_fin's streaming grid reaches its cap of 512 and
# workgroups 0 and 1 walk a second time (tiles 512 and 513: the last, ragged tile with its planted rows lies in that walk)
MLP_FC2_M = MLP_FUSED_M + (16417,)
CAST_N = (1, 7, 128, 128 * 65539 + 3)

# ---- the fp32 bars: 8 x the measured sensitivity (the worst output of the op, in the measure the GPU test applies to it: per row for token-major outputs, per tensor
# for reductions), at the op's largest listed shape with the plants in (wgrad_jobs: the worst of all its listed shapes), rounded UP to one digit.  Measured values: DESIGN.md 7.3, 7.5;
# tests/test_dense_ops_cpu.py::test_fp32_sensitivity_is_within_the_bars re-measures on every run.  None may exceed 1e-4 (what tests/test_gpu_ops.py holds).
BAR32 = {
    "linear": 2e-5,
    "linear_tanh": 6e-5,
    "linear_res": 7e-6,
    "dgrad": 2e-5,
    "dgrad_wg": 2e-5,
    "wgrad": 4e-6,
    "wgrad_jobs": 3e-6,
    "mlp_fwd": 3e-5,
    "mlp_bwd": 2e-5,
    "mlp_fused": 9e-6,
    "mlp_fc2": 9e-6,
}
# ---- bf16 mode: the measured distance between the fp64 reference and the same reference with the 16-bit roundings in (`Rounded`), same measure, same shape, rounded
# UP (one digit; mlp_bwd two, since 2e-2 would lift its bar past 3e-2); c[op] = max(BAR32[op], 2 x DIST16[op]) is the term beside the output's own bf16 ulp.  No c
# may exceed 3e-2 (what tests/test_gpu_ops.py holds).  linear_res has no 16-bit point: its c is its fp32 bar.
DIST16 = {
    "linear": 5e-3,
    "linear_tanh": 1e-2,
    "linear_res": 0.0,
    "dgrad": 5e-3,
    "dgrad_wg": 6e-3,
    "wgrad": 2e-3,
    "wgrad_jobs": 4e-3,
    "mlp_fwd": 5e-3,
    "mlp_bwd": 1.3e-2,
    "mlp_fused": 9e-3,
    "mlp_fc2": 9e-3,
}


def c16(op):
    return max(BAR32[op], 2 * DIST16[op])


# The packed-fp16 GELU / GELU' of the bf16 MLP kernels against the exact erf form, as documented beside gelu_pairs_h / gelu_grad_pairs_h in csrc/common.h (from
# tests/studies/f16_gelu_study.py): rms errors, which `Rounded` applies with a fixed pseudo-random sign to every element of H / Phi / GELU'
GELU_H_RMS = 4.7e-4
GELU_GRAD_RMS = 3.3e-4


def gen(*key):
    return torch.Generator().manual_seed(20261020 + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def rel_err(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def row_err(got, ref):
    """token-major outputs: the row's largest error over the row's own largest |ref|, the worst row -> (error, row)"""
    got, ref = got.detach().double(), ref.detach().double()
    e = (got - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-300)
    k = int(e.argmax())
    return float(e[k]), k


def row_excess(got, ref):
    """bf16 stored token-major outputs: per element |got - ref| - 2^-8 |ref|, over the row's own largest |ref|, the worst row -> (excess, row)"""
    got, ref = got.detach().double(), ref.detach().double()
    e = ((got - ref).abs() - 2.0 ** -8 * ref.abs()).amax(1) / ref.abs().amax(1).clamp_min(1e-300)
    k = int(e.argmax())
    return float(e[k]), k


class Exact:
    """no rounding: the reference itself"""
    rounded = False

    @staticmethod
    def bf(t):
        return t

    h = bf

    @staticmethod
    def noise(t, rms, key):
        return t


class Rounded:
    """the 16-bit storage points: bf16 (`bf`), fp16 (`h`), and the documented error of the packed-fp16 GELU forms (`noise`)"""
    rounded = True

    @staticmethod
    def bf(t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def h(t):
        return t.to(torch.float16).to(t.dtype)

    @staticmethod
    def noise(t, rms, key):
        sign = torch.randint(0, 2, t.shape, generator=gen(99, key)).to(t.dtype) * 2 - 1
        return t + rms * sign


# ------------------------------------------------------------------------------------------------ planted rows, LayerNorm
PLANT_KINDS = ("const", "zero", "tiny", "mean32", "big")


def second_walk_row(M, tile=32, grid=256):
    """first row of the first tile of a workgroup's second walk (persistent kernels: `grid` workgroups x contiguous ranges of ceil(tiles / grid) tiles of `tile` rows:
    workgroup 0's second tile is tile 1), or None where every workgroup has one tile"""
    return tile if (M + tile - 1) // tile > grid else None


def plant(x, g, second=None):
    """x [M,128] -> (x with the five planted rows in the first tile, in the last (ragged) tile and at row `second`, {kind: [rows]}).  A set is const, zero, tiny,
    mean32, big on consecutive rows (ascending from 0 and from `second`, descending from M - 1: the very last row is a constant one)."""
    M = x.shape[0]
    x = x.clone()
    where = {k: [] for k in PLANT_KINDS}
    used = set()

    def put(row, kind, value):
        if 0 <= row < M and row not in used:
            used.add(row)
            where[kind].append(row)
            r = torch.randn(128, generator=g)
            x[row] = {"const": torch.full((128,), value), "zero": torch.zeros(128), "tiny": 1e-3 * r, "mean32": 32 + r, "big": 1e3 * r}[kind]

    for k, kind in enumerate(PLANT_KINDS):
        put(k, kind, 0.75)
    if second is not None and second + 5 <= M:
        for k, kind in enumerate(PLANT_KINDS):
            put(second + k, kind, 0.75)
    for k, kind in enumerate(PLANT_KINDS):
        put(M - 1 - k, kind, -3.0)
    return x, where


def ln_stats(x):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + LN_EPS)
    return xc * rstd, rstd


def ln(x, g, b):
    return ln_stats(x)[0] * g + b


def ln_bwd(dxn, x, g):
    """hand-written LayerNorm backward -> (dx, dgamma, dbeta); held to autograd by tests/test_dense_ops_cpu.py"""
    xhat, rstd = ln_stats(x)
    d = dxn * g
    dx = rstd * (d - d.mean(-1, keepdim=True) - xhat * (d * xhat).mean(-1, keepdim=True))
    return dx, (dxn * xhat).sum(0), dxn.sum(0)


def ln_params(g):
    return torch.rand(128, generator=g) + 0.5, 0.1 * torch.randn(128, generator=g)


def to(ops, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in ops.items()}


def stored(ops, cd, f16=()):
    """the operands as the device holds them in mode `cd`, as fp32 tensors: in bf16 mode the tensors of the model dtype (named in ops["_model"]) are rounded to bf16,
    those in `f16` to fp16; everything else (biases, LayerNorm parameters, layer scales) is fp32 in both modes"""
    out = dict(ops)
    if cd == "bf16":
        for n in ops["_model"]:
            if ops[n] is not None:
                out[n] = ops[n].to(torch.float16 if n in f16 else torch.bfloat16).float()
    return out


# ------------------------------------------------------------------------------------------------ linear, linear_res
@functools.lru_cache(maxsize=4)        # (a case's operands are shared by the two dtypes' tests, which run back to back)
def linear_inputs(use_ln, N, act, M):
    g = gen(1, use_ln, N, act, M)
    a = torch.randn(M, 128, generator=g)
    where = {}
    if use_ln:
        a, where = plant(a, g, second_walk_row(M))
    w = torch.randn(N, 128, generator=g) * 128 ** -0.5
    bias = 0.1 * torch.randn(N, generator=g)
    if act:
        bias[5], bias[6] = 26.0, -26.0                    # |z| > 20 on every token: tanh = +-1 exactly (large WEIGHTS would do it too, but multiply the bf16 rounding of
    gm, bt = ln_params(g)                                 # LN(a) into a z error of 0.05 where tanh is steep: 9e-2 of the row between two evaluations of the REFERENCE)
    return dict(a=a, w=w, bias=bias, g=gm if use_ln else None, b=bt if use_ln else None, where=where, _model=("a", "w"))


def linear_ref(a, w, bias, g, b, act, R=Exact):
    """16-bit points (bf16 mode): LN(a) as the GEMM operand.  -> y, xn (the unrounded LN(a): xn_out's own rounding is the output's ulp), z (the pre-activation)"""
    out = {}
    if g is not None:
        out["xn"] = ln(a, g, b)
        a = R.bf(out["xn"])
    z = a @ w.T + bias
    out["z"] = z
    out["y"] = torch.tanh(z) if act else z
    return out


@functools.lru_cache(maxsize=4)        # (a case's operands are shared by the two dtypes' tests, which run back to back)
def linear_res_inputs(M):
    g = gen(2, M)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(a=r(M, 128), w=r(128, 128) * 128 ** -0.5, bias=0.1 * r(128), ls=0.5 + torch.rand(128, generator=g), resid=r(M, 128), _model=("a", "w", "resid"))


def linear_res_ref(a, w, bias, ls, resid, R=Exact):
    """no 16-bit point: fp32 accumulators straight into the epilogue"""
    return dict(out=resid + ls * (a @ w.T + bias))


# ------------------------------------------------------------------------------------------------ data gradient + LayerNorm backward (+ fused weight gradient)
def wg_ranges(M, tile=32, grid=256):
    """token ranges [(first row, end row)] of the workgroups of a persistent launch that own a tile (launch_dgrad_r, k_gemm2.hip: `grid` workgroups x contiguous
    ranges of ceil(tiles / grid) tiles; kasf_launch_mlp_bwd_q, k_mlp2.hip: the same with grid 64)"""
    tiles = (M + tile - 1) // tile
    per = (tiles + min(tiles, grid) - 1) // min(tiles, grid)
    return [(t0 * tile, min((t0 + per) * tile, M)) for t0 in range(0, tiles, per)]


@functools.lru_cache(maxsize=4)        # (a case's operands are shared by the two dtypes' tests, which run back to back)
def dgrad_inputs(Kd, M, proj=False):
    g = gen(3, Kd, M)
    r = lambda *s: torch.randn(*s, generator=g)
    x, where = plant(r(M, 128), g, second_walk_row(M))
    gm, bt = ln_params(g)
    W = r(Kd, 128) * 128 ** -0.5                          # the forward weight [out = Kd, in = 128]
    ops = dict(x=x, dy=r(M, Kd), add=r(M, 128), resid=r(M, 128), prev=r(M, 128), wt=W.T.contiguous(), g=gm, b=bt, where=where,
               _model=("x", "dy", "add", "resid", "prev", "wt", "o"), o=None)
    if proj:
        ops.update(o=r(M, 128), pw=r(128, 128) * 128 ** -0.5, pb=0.1 * r(128), pls=0.5 + torch.rand(128, generator=g))
    return ops


def dgrad_ref(dy, wt, add, x, g, resid, prev, b, R=Exact):
    """out = [resid] + [prev] + LNbwd(dy wt^T [+ add]).  16-bit point: the GEMM's dxn tile (bf16 in LDS) before `add` joins it in fp32."""
    dxn = R.bf(dy @ wt.T)
    if add is not None:
        dxn = dxn + add
    dx, dgamma, dbeta = ln_bwd(dxn, x, g)
    out = dx + (resid if resid is not None else 0) + (prev if prev is not None else 0)
    return dict(out=out, dgamma=dgamma, dbeta=dbeta, xn=ln(x, g, b))


def ranged_tn(A, B, ranges, R):
    """A^T B over the token axis; `Rounded`: one bf16 rounding of every token range's partial product (the per-workgroup bf16 partial tiles)"""
    if not R.rounded:
        return A.T @ B
    return sum(R.bf(A[r0:r1].T @ B[r0:r1]) for r0, r1 in ranges)


def dgrad_wg_ref(dy, wt, add, x, g, resid, prev, b, bias, o, pw, pb, pls, R=Exact):
    """dgrad_ref + dw [Kd,128] = dy^T LN(x) (+ dbias = colsum(dy)) (+ the proj gradients of the PROJ form).  16-bit points on top of dgrad_ref's: LN(x) as the
    weight gradient's operand, and one bf16 partial tile of dw (and of G = resid^T o) per token range of launch_dgrad_r."""
    out = dgrad_ref(dy, wt, add, x, g, resid, prev, b, R)
    ranges = wg_ranges(x.shape[0])
    out["dw"] = ranged_tn(dy, R.bf(out["xn"]), ranges, R)
    if bias:
        out["dbias"] = dy.sum(0)
    if o is not None:
        G, c = ranged_tn(resid, o, ranges, R), resid.sum(0)
        out.update(dproj_w=pls[:, None] * G, dproj_b=pls * c, dproj_ls=(pw * G).sum(1) + pb * c)
    return out


# ------------------------------------------------------------------------------------------------ weight gradient
def wgrad_splits(N, K, M):
    """wgrad_T (k_gemm.hip): the split count of the launch -> (splits, floats of `partial` the fixed-order path needs with a bias gradient)"""
    tiles = (N // 128) * (K // 128)
    splits = max(1, min((248 + tiles - 1) // tiles, (M + 127) // 128))
    sl = ((M + splits - 1) // splits + 127) // 128 * 128
    splits = (M + sl - 1) // sl
    return splits, splits * N * K + splits * N


@functools.lru_cache(maxsize=4)        # (a case's operands are shared by the two dtypes' tests, which run back to back)
def wgrad_inputs(N, K, use_ln, M):
    g = gen(4, N, K, use_ln, M)
    x = torch.randn(M, K, generator=g)
    where = {}
    if use_ln:
        x, where = plant(x, g, 128 if M > 256 else None)      # (row 128: the second 128-row tile of the first split)
    gm, bt = ln_params(g)
    return dict(g=torch.randn(M, N, generator=g), x=x, gm=gm if use_ln else None, bt=bt if use_ln else None, where=where, _model=("g", "x"))


def wgrad_ref(g, x, gm, bt, R=Exact):
    """dw [N,K] = g^T LN?(x), dbias = colsum(g).  16-bit point: LN(x) as the GEMM operand (the partial tiles of kasf_op_wgrad are fp32)"""
    xn = R.bf(ln(x, gm, bt)) if gm is not None else x
    return dict(dw=g.T @ xn, dbias=g.sum(0))


# ------------------------------------------------------------------------------------------------ several weight gradients in one launch (bf16)
def jobs_splits(M, Ns):
    """kasf_launch_wgrad_jobs (k_gemm.hip) at full width: -> (splits, slice): target 248 workgroups over the jobs' 128-column tiles, slices of whole WG_BM = 128-row
    tiles.  Split z streams rows [z slice, min((z + 1) slice, M)) as 64-row ring tiles and a register tail; every job has the same splits."""
    tiles = sum(N // 128 for N in Ns)
    splits = min((248 + tiles - 1) // tiles, (M + 127) // 128)
    sl = ((M + splits - 1) // splits + 127) // 128 * 128
    return (M + sl - 1) // sl, sl


def jobs_partial_floats(M, Ns, fin_job):
    """the floats of `partial` the launcher asks: a tile [N][128] per split and job, and one row [128] per split behind the fin job's tiles"""
    splits = jobs_splits(M, Ns)[0]
    return sum(splits * N * 128 for N in Ns) + (splits * Ns[fin_job] if fin_job >= 0 else 0)


def jobs_cases(mix):
    """[(M, parts)] of one mix"""
    return [(M, JOBS_PARTS[mix][k % len(JOBS_PARTS[mix])]) for k, M in enumerate(JOBS_M[mix])]


@functools.lru_cache(maxsize=2)
def jobs_inputs(mix, M, parts, redraw=0):
    """the operands as the device holds them (fp32 tensors of bf16 values for G, X, the reductions' parts and the ext tiles; fp32 for the fin vectors and the ext rows).
    redraw: jobs 1.. are drawn from another seed, job 0 and everything else is unchanged (the isolation case)."""
    Ns, fin_job, reds, ext = JOBS_MIXES[mix]
    key = (7, list(JOBS_MIXES).index(mix), M, parts)
    g = gen(*key)
    bf = lambda t: t.to(torch.bfloat16).float()
    r = lambda *s: torch.randn(*s, generator=g)
    G, X = [bf(r(M, Ns[0]))], [bf(r(M, 128))]
    ops = dict(W=r(128, 128) * 128 ** -0.5, bias=0.1 * r(128), ls=0.5 + torch.rand(128, generator=g), Ns=Ns, fin_job=fin_job)
    ops["red"] = [bf(r(parts if k == 0 else 33, e)) for k, e in enumerate(reds)]
    ops["ext_part"], ops["ext_brow"] = (bf(4 * r(parts, 128, 128)), 4 * r(parts, 128)) if ext else (None, None)
    if redraw:
        g = gen(*key, redraw)
    for N in Ns[1:]:
        G.append(bf(r(M, N)))
        X.append(bf(r(M, 128)))
    ops.update(G=G, X=X)
    return ops


def jobs_sel(i, dtype):
    """the arguments of wgrad_jobs_ref in `dtype`"""
    c = lambda t: None if t is None else t.to(dtype)
    return [c(t) for t in i["G"]], [c(t) for t in i["X"]], i["fin_job"], c(i["W"]), c(i["bias"]), c(i["ls"]), [c(t) for t in i["red"]], c(i["ext_part"]), c(i["ext_brow"])


def ls_algebra(Gm, c, W, bias, ls):
    """the layer-scaled proj weight from the unscaled G = g^T x and c = colsum(g): -> dW, db, dls (k_wgrad_finish_jobs; held to autograd by dgrad_wg_ref's test)"""
    return ls[:, None] * Gm, ls * c, (W * Gm).sum(1) + bias * c


def wgrad_jobs_ref(G, X, fin_job, W, bias, ls, red, ext_part, ext_brow, R=Exact):
    """dw<j> [N_j,128] = G_j^T X_j per job (the fin job: the layer-scale algebra, with db and dls); red<k> = the sum of reduction k's parts; the ext job: the algebra
    on the sum of its tiles and rows (ext_dw, ext_db, dls).  16-bit point: ONE bf16 tile per job and token split of jobs_splits.  The rows of colsum(G) per split
    are fp32, and the reductions' parts and the ext tiles are bf16 INPUTS summed in fp32: red<k>, db, ext_dw, ext_db and the ext job's dls have no 16-bit point."""
    splits, sl = jobs_splits(G[0].shape[0], [g.shape[1] for g in G])
    out = {}
    for j, (g, x) in enumerate(zip(G, X)):
        Gm = sum(R.bf(g[z * sl:(z + 1) * sl].T @ x[z * sl:(z + 1) * sl]) for z in range(splits)) if R.rounded else g.T @ x
        if j == fin_job:
            out[f"dw{j}"], out["db"], out["dls"] = ls_algebra(Gm, g.sum(0), W, bias, ls)
        else:
            out[f"dw{j}"] = Gm
    for k, p in enumerate(red):
        out[f"red{k}"] = p.sum(0)
    if ext_part is not None:
        out["ext_dw"], out["ext_db"], out["dls"] = ls_algebra(ext_part.sum(0), ext_brow.sum(0), W, bias, ls)
    return out


def jobs_no16(name, i):
    """the outputs of wgrad_jobs_ref that no 16-bit point lies in front of"""
    return name in ("db", "ext_dw", "ext_db") or name.startswith("red") or (name == "dls" and i["ext_part"] is not None)


# ------------------------------------------------------------------------------------------------ MLP
def gelu(z):
    return 0.5 * z * (1 + torch.erf(z * 2 ** -0.5))


def gelu_grad(z):
    return 0.5 * (1 + torch.erf(z * 2 ** -0.5)) + z * torch.exp(-0.5 * z * z) * (2 * math.pi) ** -0.5


@functools.lru_cache(maxsize=4)        # (a case's operands are shared by the two dtypes' tests, which run back to back)
def mlp_inputs(M, grid=256):
    g = gen(5, M, grid)
    r = lambda *s: torch.randn(*s, generator=g)
    x, where = plant(r(M, 128), g, second_walk_row(M, 32, grid))
    gm, bt = ln_params(g)
    W1, b1 = r(512, 128) * 128 ** -0.5, 0.1 * r(512)
    W1[7] *= 3.0                                          # unit 7: z of deviation ~3, beyond +-6 on a few per cent of the tokens (erf tail)
    W1[9] *= 5.0                                          # unit 9: deviation ~5, beyond +-12 on 2 % (far past the packed-fp16 form's clamp at |z| = 4; fp16 range 65504)
    b1[7], b1[9] = 0.5, -0.5                              # (x 8 reaches +-12 on a tenth, but the unit then multiplies LN(x)'s bf16 rounding into 2e-2 of a row of H / dZ)
    W2, ls = r(128, 512) * 512 ** -0.5, 0.5 + torch.rand(128, generator=g)
    return dict(x=x, gm=gm, bt=bt, W1=W1, b1=b1, W2=W2, b2=0.1 * r(128), ls=ls, gout=r(M, 128), W2s=ls[:, None] * W2, where=where,
                _model=("x", "W1", "W2", "W2s", "gout"))                 # W2s: the layer-scaled copy the backward kernels are handed (transposed) as w2t_scaled


def mlp_fwd_ref(x, gm, bt, W1, b1, W2, b2, ls, R=Exact):
    """out = x + ls (GELU(LN(x) W1^T + b1) W2^T + b2).  16-bit points (bf16 mode, k_mlp_fwd_s): LN(x) as xn_out / GEMM1 operand (bf16), z and H in fp16 (W2 is an
    fp16 operand already), the packed-fp16 GELU's documented error on H."""
    xn = ln(x, gm, bt)
    z = R.h(R.bf(xn) @ W1.T + b1)
    H = R.h(R.noise(gelu(z), GELU_H_RMS, 1))
    return dict(out=x + ls * (H @ W2.T + b2), xn=xn, z=z, H=H)


def mlp_bwd_ref(x, gout, gm, bt, W1, b1, W2s, R=Exact, xn_op=None, fused_M_grid=None):
    """Backward of mlp_fwd_ref for the upstream gradient gout, written out (held to autograd by tests/test_dense_ops_cpu.py):
         dH = gout W2s, W2s = ls[:, None] W2 (a packed operand of its own);  dZ = dH GELU'(z);  dA = dZ W1;  g_in = gout + LNbwd(dA);  dW1 = dZ^T LN(x), db1 = colsum(dZ);
         dW2u = gout^T H (UNSCALED: dW2 = ls[:, None] dW2u), gsum = colsum(gout) (db2 = ls gsum).
    16-bit points, generic kernel (k_mlp_bwd<bf16> + kasf_op_wgrad): LN(x) as operand, H and dZ as stored (and as operands), dA where it passes the bf16 tile
    in front of the LayerNorm backward.  Fused kernels (fused_M_grid = 64; k_mlp_bwd_s + k_lnbwd_sum4_fin): xn_op = the LN(x) the forward stored is the operand, H and
    dZ are bf16 operands, GELU' carries the packed-fp16 form's documented error, dA is the sum of four bf16 partials (one per hidden quarter) and dW1 / dW2u the
    sum of one bf16 partial tile per token range of kasf_launch_mlp_bwd_q."""
    xn = ln(x, gm, bt)
    xo = R.bf(xn) if xn_op is None else xn_op
    z = xo @ W1.T + b1
    fused = fused_M_grid is not None
    H = R.bf(R.noise(gelu(z), GELU_GRAD_RMS, 2) if fused else gelu(z))
    dZ = R.bf((gout @ W2s) * (R.noise(gelu_grad(z), GELU_GRAD_RMS, 3) if fused else gelu_grad(z)))
    if fused and R.rounded:
        dA = sum(R.bf(dZ[:, q * 128:(q + 1) * 128] @ W1[q * 128:(q + 1) * 128]) for q in range(4))
    else:
        dA = R.bf(dZ @ W1)
    dx, dgamma, dbeta = ln_bwd(dA, x, gm)
    ranges = wg_ranges(x.shape[0], 32, fused_M_grid) if fused else None
    out = dict(g_in=gout + dx, dgamma=dgamma, dbeta=dbeta, H=H, dZ=dZ, db1=dZ.sum(0), gsum=gout.sum(0))
    if fused:
        out.update(dW1=ranged_tn(dZ, xo, ranges, R), dW2u=ranged_tn(gout, H, ranges, R))
    else:
        out.update(dW1=dZ.T @ xo, dW2u=gout.T @ H)
    return out


def mlp_fc2_inputs(M):
    """the operands of kasf_op_mlp_bwd_fused_fc2 as bf16 mode holds them: those of the fused backward, with W2 the fp32 MASTER of fc2 (the layer-scale algebra reads
    it; W2s stays the bf16 copy of ls W2 that the data path multiplies by)"""
    i = stored(mlp_inputs(M, 64), "bf16")
    i["W2"] = mlp_inputs(M, 64)["W2"]
    return i


def mlp_fc2_ref(x, gout, gm, bt, W1, b1, W2s, W2, b2, ls, R=Exact, xn_op=None):
    """the fused backward (mlp_bwd_ref, fused_M_grid = 64) with fc2 finished as a backward stage finishes it: dW2 = ls dW2u (SCALED), db2 = ls gsum,
    dls2 = <W2, dW2u> + b2 gsum.  No 16-bit point beyond mlp_bwd_ref's (the algebra runs in fp32 on the summed tiles); db2 has none at all."""
    out = mlp_bwd_ref(x, gout, gm, bt, W1, b1, W2s, R, xn_op, 64)
    out["dW2"], out["db2"], out["dls2"] = ls_algebra(out["dW2u"], out["gsum"], W2, b2, ls)
    return out


# ------------------------------------------------------------------------------------------------ scratch of the column sink (kasf_op_sink_scratch_floats, restated)
def sink_floats(*takes):
    """KasfColSink::take: (rows, row length) per request, each rounded up to 64 floats"""
    return sum((rows * ld + 63) // 64 * 64 for rows, ld in takes)


def fc2_scratch_floats(M):
    """kasf_launch_mlp_bwd_q: one row of db1 [512] per token range that owns a tile, one row of dgamma | dbeta | colsum(g) [384] per streaming workgroup (<= 512)"""
    return sink_floats((len(wg_ranges(M, 32, 64)), 512), (min((M + 31) // 32, 512), 384))


def mlp_bwd_rows(cd, M):
    """k_mlp_bwd's grid: tiles of 32 (fp32) / 64 (bf16) tokens, one row of dgamma | dbeta each"""
    return (M + 31) // 32 if cd == "fp32" else (M + 63) // 64


def dgrad_rows(cd, case, M):
    """the rows of dgamma | dbeta of kasf_op_dgrad_lnbwd_rows: bf16, the four persistent instantiations of k_dgrad_r: the workgroups that own a tile; otherwise
    k_dgrad_lnbwd's grid of 64-row tiles"""
    persistent = cd == "bf16" and tuple(case) in ((384, False, True, False, True), (128, False, True, False, True), (256, False, False, True, True),
                                                  (256, True, True, False, False))
    return len(wg_ranges(M)) if persistent else (M + 63) // 64


def gcn_bwd_rows(M):
    """k_gcn_bwd1's grid: 16 tokens per workgroup, capped at 512; one row of dls1 [128] each"""
    return min(512, max(1, (M * 16 + 255) // 256))


# ------------------------------------------------------------------------------------------------ cast
@functools.lru_cache(maxsize=2)
def cast_inputs(n):
    """fp32 values whose bf16 rounding exercises ties (to even, both ways), the carry into the exponent, +-0, +-inf, NaN, the largest finite values and subnormals"""
    g = gen(6, n)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 30, (n,), generator=g).float())
    special = torch.tensor([0.0, -0.0, math.inf, -math.inf, math.nan, 3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38, 1.0 + 2.0 ** -8,
                            1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 2.0 - 2.0 ** -9, 1e-40, -1e-45, 65504.0, 2.0 ** -126])
    k = min(n, special.numel())
    x[n - k:] = special[:k]
    return x


# ------------------------------------------------------------------------------------------------ the CPU measurements behind BAR32 and DIST16
def _split(keys_rows, r_a, r_b, skip=()):
    """{output: distance}: per row for the token-major outputs named in keys_rows, per tensor for the rest; z and `skip` are not outputs"""
    return {k: (row_err(r_a[k], r_b[k])[0] if k in keys_rows else rel_err(r_a[k], r_b[k])) for k in r_b if k != "z" and k not in skip}


def _f(ops, dtype, names):
    return [ops[n].to(dtype) if ops[n] is not None else None for n in names]


def measure(which):
    """which = 'fp32': op -> {output: distance(fp32 evaluation, fp64 evaluation)} on fp32 operands; 'bf16': op -> {output: distance(`Rounded` fp64 evaluation, fp64
    evaluation)} on the operands as bf16 mode stores them.  Each op at its largest listed shape(s), the worst over the listed configurations."""
    f32 = which == "fp32"
    cd = "fp32" if f32 else "bf16"
    lo = torch.float32 if f32 else torch.float64
    R = Exact if f32 else Rounded
    out = {}

    def worst(op, d):
        cur = out.setdefault(op, {})
        for k, v in d.items():
            cur[k] = max(cur.get(k, 0.0), v)

    for use_ln, N, act in LINEAR_CASES:
        i = stored(linear_inputs(use_ln, N, act, max(LINEAR_M)), cd)
        n = ("a", "w", "bias", "g", "b")
        worst("linear_tanh" if act else "linear", _split(("y", "xn"), linear_ref(*_f(i, lo, n), act, R), linear_ref(*_f(i, torch.float64, n), act)))
    i = stored(linear_res_inputs(max(LINEAR_M)), cd)
    n = ("a", "w", "bias", "ls", "resid")
    worst("linear_res", _split(("out",), linear_res_ref(*_f(i, lo, n), R), linear_res_ref(*_f(i, torch.float64, n))))
    for Kd, use_add, use_resid, acc, want_xn in DGRAD_CASES:
        i = stored(dgrad_inputs(Kd, max(DGRAD_M)), cd)
        sel = lambda dt: [i[k].to(dt) if use else None for k, use in (("dy", 1), ("wt", 1), ("add", use_add), ("x", 1), ("g", 1), ("resid", use_resid), ("prev", acc), ("b", 1))]
        worst("dgrad", _split(("out", "xn"), dgrad_ref(*sel(lo), R), dgrad_ref(*sel(torch.float64))))
    for form, (Kd, use_resid, acc, bias, proj) in WG_FORMS.items():
        i = stored(dgrad_inputs(Kd, max(DGRAD_WG_M), proj), cd)
        sel = lambda dt: [i[k].to(dt) if use else None for k, use in (("dy", 1), ("wt", 1), ("add", bias), ("x", 1), ("g", 1), ("resid", use_resid), ("prev", acc), ("b", 1))] \
            + [bias] + [i[k].to(dt) if proj else None for k in ("o", "pw", "pb", "pls")]
        worst("dgrad_wg", _split(("out", "xn"), dgrad_wg_ref(*sel(lo), R), dgrad_wg_ref(*sel(torch.float64))))
    for N, K in WGRAD_NK:
        for use_ln in ((1, 0) if K == 128 else (0,)):
            i = stored(wgrad_inputs(N, K, use_ln, max(WGRAD_M)), cd)
            n = ("g", "x", "gm", "bt")
            worst("wgrad", _split((), wgrad_ref(*_f(i, lo, n), R), wgrad_ref(*_f(i, torch.float64, n))))
    for mix in JOBS_MIXES:                                 # (a bf16 entry: the operands are bf16 values in both evaluations; every listed shape: they are small)
        for M, parts in jobs_cases(mix):
            i = jobs_inputs(mix, M, parts)
            worst("wgrad_jobs", _split((), wgrad_jobs_ref(*jobs_sel(i, lo), R), wgrad_jobs_ref(*jobs_sel(i, torch.float64))))
    i = stored(mlp_inputs(max(MLP_FWD_M[cd])), cd, f16=("W2",))
    n = ("x", "gm", "bt", "W1", "b1", "W2", "b2", "ls")
    worst("mlp_fwd", _split(("out", "xn"), mlp_fwd_ref(*_f(i, lo, n), R), mlp_fwd_ref(*_f(i, torch.float64, n)), skip=("H",)))
    n = ("x", "gout", "gm", "bt", "W1", "b1", "W2s")
    i = stored(mlp_inputs(max(MLP_BWD_M)), cd)
    worst("mlp_bwd", _split(("g_in", "H", "dZ"), mlp_bwd_ref(*_f(i, lo, n), R), mlp_bwd_ref(*_f(i, torch.float64, n))))
    i = stored(mlp_inputs(max(MLP_FUSED_M), 64), cd)
    worst("mlp_fused", _split(("g_in",), mlp_bwd_ref(*_f(i, lo, n), R, None, 64), mlp_bwd_ref(*_f(i, torch.float64, n), Exact, None, 64), skip=("H", "dZ")))
    out["mlp_fc2"] = measure_fc2(which)
    return out


def measure_fc2(which):
    """measure()'s entry of the fc2 form, at its largest listed shape; dW2u and gsum are not outputs of that entry (dW2 and db2 take their slots)"""
    f32 = which == "fp32"
    i = mlp_fc2_inputs(max(MLP_FC2_M)) if not f32 else dict(mlp_inputs(max(MLP_FC2_M), 64))
    n = ("x", "gout", "gm", "bt", "W1", "b1", "W2s", "W2", "b2", "ls")
    return _split(("g_in",), mlp_fc2_ref(*_f(i, torch.float32 if f32 else torch.float64, n), Exact if f32 else Rounded),
                  mlp_fc2_ref(*_f(i, torch.float64, n)), skip=("H", "dZ", "dW2u", "gsum"))
