"""The GCN mixer on its own (include/kasf.h: kasf_op_gcn_fwd / kasf_op_gcn_bwd, the eight kernels of csrc/k_gcn.hip) against fp64 torch math of the same
operation on the dtype-rounded operands: skeleton / top-k adjacency with ties kept, D^-1/2 A D^-1/2, BatchNorm with explicit mean and biased variance, ReLU,
layer scale, residual, and autograd of all of it.

How the comparison is set up (the same in every test below):
  * Temporal cases use integer-valued LN(x) rows in [-3, 3]: every 128-term similarity is an integer of magnitude <= 1,152, exact in bf16 storage, in the fp32
    MFMA accumulation and in fp64, so the stored adjacency mask must equal the reference's `>=` decision BIT FOR BIT, ties included, in both dtypes.  The seed
    is chosen on the CPU so that at least one row keeps more than k neighbours (impossible only when n_frames == k).
  * `y` is an OUTPUT of the forward entry (compared with the reference's own y) and an OPERAND of the backward entry, and the BatchNorm statistics are those of
    y as stored (kasf.h).  Everything after y -- statistics, out, gradients -- is therefore referenced on the stored y (the reference's y with the stored values
    substituted, gradients still flowing to U and V).  Without that, a bf16 rounding of y flips the ReLU of every element with |z| below 2^-9 |y|, and r, a
    product with a 0 / 1 gate, differs by O(1) at those elements whatever the kernels do.
  * The ReLU gate is a discontinuity: an element whose reference pre-activation z lies within the fp32 resolution of the kernel's own z (`_gate_margin`: 1e-5 of
    the magnitude of the three terms of z, plus the analytic sensitivity of z to fp32 partial sums in the variance) has no well-defined gate.  The upstream
    gradient g is set to ZERO at those elements before the backward runs (a few per million; the fraction is asserted), so that both sides give 0 there.
  * Outputs that are accumulated into (dls1, d_bn_w, d_bn_b) start at 1; buffers that are written start at a sentinel.
"""
import ctypes as C
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import kasf_oracle as O
from tests.gpu_util import DT, decode_masks, ptr, rel_err, stream

pytestmark = pytest.mark.gpu
TOL = {"fp32": 1e-4, "bf16": 3e-2}
J, CH = 17, 128
MOMENTUM = 0.25                 # not BatchNorm1d's default: the argument has to arrive
SENTINEL = 7.0

TEMPORAL_SHAPES = [(9, 2), (27, 3), (81, 2),                # the templated kernels
                   (4, 2), (5, 2),                          # k = 4 with T = 4: every frame is a neighbour
                   (16, 2), (17, 2), (33, 2), (96, 1),      # the generic kernel with 3 mask words: block and tile edges
                   (97, 1), (130, 1), (256, 1),             # wide masks
                   (27, 70),                                # 1,190 tracks: a templated workgroup owns more than one track
                   (50, 61),                                # 1,037 tracks: the generic kernel, two tracks per workgroup
                   (81, 46)]                                # several tracks per workgroup at the three-per-CU LDS size
SPATIAL_SHAPES = [(27, 2),                                  # the ordinary case
                  (4, 1),                                   # 68 tokens: a partly filled last workgroup
                  (9, 117),                                 # 17,901 tokens: agg_spatial's 1,024-workgroup cap with a ragged second pass; bwd1's pair loop with has1 false for part of the grid
                  (27, 143)]                                # 65,637 tokens: just past apply's 4,096-workgroup cap
PARITY_CASES = [(1, T, B) for T, B in TEMPORAL_SHAPES] + [(0, T, B) for T, B in SPATIAL_SHAPES]


@pytest.fixture(scope="module")
def lib():
    from kasportsformer_amd import _lib
    return _lib.load()


_KEEP = []


@pytest.fixture(autouse=True)
def _keepalive():
    """Device tensors handed to the (asynchronous) launches must outlive them."""
    _KEEP.clear()
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _dev(t, dtype):
    d = t.to(dtype).cuda().contiguous()
    _KEEP.append(d)
    return d


def _new(shape, dtype, fill=SENTINEL):
    d = torch.full(shape, fill, device="cuda", dtype=dtype)
    _KEEP.append(d)
    return d


def _back(t):
    return t.detach().double().cpu()


# ------------------------------------------------------------------------------------------------ layout
def _group(t, mode, B, T):
    """[M, C] in [batch][frame][joint] token order -> [groups, nodes, C]: spatial groups = (clip, frame), nodes = joints; temporal groups = (clip, joint), nodes = frames"""
    v = t.view(B, T, J, t.shape[-1])
    return v.reshape(B * T, J, -1) if mode == 0 else v.transpose(1, 2).reshape(B * J, T, -1)


def _ungroup(t, mode, B, T):
    return t.reshape(B * T * J, -1) if mode == 0 else t.view(B, J, T, -1).transpose(1, 2).reshape(B * T * J, -1)


def _count(mode, B, T):
    return B * T * CH if mode == 0 else B * J * CH


def _adjacency(xn_g, mode, k):
    if mode == 0:
        return O.skeleton_adjacency(J).double().expand(xn_g.shape[0], J, J)
    return O.temporal_topk_adjacency(xn_g, k)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=2)
def _inputs(mode, T, B, k, base_seed=20261017):
    """fp32 CPU tensors of one case.  Temporal: the first seed whose integer-valued xn gives a row of degree > k."""
    M = B * T * J
    nodes = J if mode == 0 else T
    for seed in range(base_seed, base_seed + 64):
        gen = torch.Generator().manual_seed(seed + 1000 * T + B)
        if mode == 1:
            xn = torch.randint(-3, 4, (M, CH), generator=gen).float()
            if k == 1:                                          # a tie at the FIRST place needs a frame equal to another: the diagonal |xn|^2 beats every other similarity otherwise
                v = xn.view(B, T, J, CH)
                v[0, 5, 2] = v[0, 0, 2]
            deg = _adjacency(_group(xn.double(), mode, B, T), mode, k).sum(-1)
            if T > k and not bool((deg > k).any()):
                continue
        else:
            xn = torch.randn(M, CH, generator=gen)
        break
    else:
        raise AssertionError("no seed with a tie at the k-th place")
    r = lambda *s: torch.randn(*s, generator=gen)
    offs = 0.5 * r(nodes)                                   # a mean per node for BatchNorm to remove
    uv = r(M, 2 * CH)
    uv[:, :CH] += _ungroup(offs.view(1, nodes, 1).expand(B * T * J // nodes, nodes, 1).contiguous(), mode, B, T)
    return dict(xn=xn, uv=uv, x_in=r(M, CH), g=r(M, CH), bn_w=0.5 + torch.rand(nodes, generator=gen), bn_b=r(nodes), ls1=r(CH),
                run_mean=0.3 * r(nodes), run_var=0.5 + torch.rand(nodes, generator=gen))


# ------------------------------------------------------------------------------------------------ fp64 reference
class Ref:
    """Forward in fp64 on the given (already dtype-rounded, fp64) operands; `y_stored` substitutes the values of y while keeping the graph to U and V."""

    def __init__(self, op, mode, T, B, k, training, y_stored=None, var_scale=1.0):
        self.mode, self.T, self.B, self.training = mode, T, B, training
        gr = lambda t: _group(t, mode, B, T)
        self.U = op["uv"][:, :CH].clone().requires_grad_(True)
        self.V = op["uv"][:, CH:].clone().requires_grad_(True)
        self.xn_d = op["xn"].clone().requires_grad_(True)           # the direct term of z; the adjacency reads op["xn"] and carries no gradient
        self.bn_w, self.bn_b, self.ls1 = (op[n].clone().requires_grad_(True) for n in ("bn_w", "bn_b", "ls1"))
        self.adj = _adjacency(gr(op["xn"]), mode, k)
        self.ahat = O.normalize_adjacency(self.adj)
        self.y0 = self.ahat @ gr(self.V) + gr(self.U)
        y = self.y0 if y_stored is None else self.y0 + (gr(y_stored) - self.y0).detach()
        self.y = y
        self.count = _count(mode, B, T)
        bmean = y.mean(dim=(0, 2))
        bvar = ((y - bmean[None, :, None]) ** 2).mean(dim=(0, 2))
        self.batch_mean, self.batch_var = bmean.detach(), bvar.detach()
        mean, var = (bmean, bvar * var_scale) if training else (op["run_mean"], op["run_var"])
        self.mean, self.var = mean, var
        self.rstd = (var + 1e-5) ** -0.5
        self.scale = self.bn_w * self.rstd
        self.shift = self.bn_b - mean * self.scale
        self.yhat = (y - mean[None, :, None]) * self.rstd[None, :, None]
        self.z = gr(self.xn_d) + self.yhat * self.bn_w[None, :, None] + self.bn_b[None, :, None]
        self.out_g = gr(op["x_in"]) + self.ls1 * torch.relu(self.z)
        self.op = op

    def flat(self, t):
        return _ungroup(t.detach(), self.mode, self.B, self.T)

    def coef(self):
        return torch.stack([self.scale, self.shift, self.mean, self.rstd], dim=1).detach()

    def running(self, momentum):
        unbiased = self.batch_var * self.count / (self.count - 1)
        return ((1 - momentum) * self.op["run_mean"] + momentum * self.batch_mean, (1 - momentum) * self.op["run_var"] + momentum * unbiased)

    def gate_margin(self):
        """|z| below which the kernel's fp32 z and this fp64 z may disagree in sign: 1e-5 of the magnitude of z's terms (fp32 rounding of scale, shift and the two
        multiply-adds: a few 2^-24 each), plus the change of z when the variance moves by (1 + rho^2) 2^-22 relative (kasf.h RANGE: fp32 partial sums)."""
        with torch.no_grad():
            bn = (self.yhat * self.bn_w[None, :, None]).abs().max()
            zmag = self.op["xn"].abs().max() + (self.y.abs() * self.scale.abs()[None, :, None]).max() + self.shift.abs().max()
            rho2 = float((self.batch_mean ** 2 / self.batch_var.clamp_min(1e-300)).max()) if self.training else 0.0
            return float(1e-5 * zmag + 4 * (1 + rho2) * 2.0 ** -22 * bn)

    def backward(self, g):
        self.out_g.backward(_group(g, self.mode, self.B, self.T))
        return dict(r=self.xn_d.grad, duv=torch.cat([self.U.grad, self.V.grad], dim=1), dls1=self.ls1.grad, d_bn_w=self.bn_w.grad, d_bn_b=self.bn_b.grad)

    def backward_by_hand(self, g, rnd=lambda t: t):
        """The BatchNorm backward written out as the kernels evaluate it (k_gcn_bwd1 / bwd2), in fp64; `rnd` is applied where the kernels STORE in the model dtype:
        r (read back by bwd2; the BatchNorm-backward sums are formed from the unrounded values) and dU | dV."""
        with torch.no_grad():
            gg = _group(g, self.mode, self.B, self.T)
            r = self.ls1 * gg * (self.z > 0)
            s0, s1 = r.sum(dim=(0, 2)), (r * self.yhat).sum(dim=(0, 2))
            dls1 = (gg * torch.relu(self.z)).sum(dim=(0, 1))
            r_st = rnd(r)
            c1, c2 = (s0 / self.count, s1 / self.count) if self.training else (torch.zeros_like(s0), torch.zeros_like(s1))
            dy = self.scale[None, :, None] * (r_st - c1[None, :, None] - self.yhat * c2[None, :, None])
            dv = self.ahat.transpose(1, 2) @ dy
            return dict(r=self.flat(r_st), duv=torch.cat([self.flat(rnd(dy)), self.flat(rnd(dv))], dim=1), dls1=dls1, d_bn_w=s1, d_bn_b=s0)


def _round_bf16(t):
    return t.to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------ running the two entries
class Run:
    """Device operands of one case and the outputs of kasf_op_gcn_fwd; .backward(g) runs kasf_op_gcn_bwd."""

    def __init__(self, lib, cd, inp, mode, T, B, k, training):
        from kasportsformer_amd import _lib
        self.lib, self.cd, self.mode, self.T, self.B, self.training = lib, cd, mode, T, B, training
        code, dt = DT[cd]
        M, nodes = B * T * J, (J if mode == 0 else T)
        self.M, self.nodes = M, nodes
        d = self.d = {n: _dev(inp[n], dt) for n in ("xn", "uv", "x_in")}
        for n in ("bn_w", "bn_b", "ls1"):
            d[n] = _dev(inp[n], torch.float32)
        self.run_mean, self.run_var = _new((256,), torch.float32), _new((256,), torch.float32)
        self.run_mean[:nodes] = inp["run_mean"].cuda()
        self.run_var[:nodes] = inp["run_var"].cuda()
        self.run0 = (self.run_mean.clone(), self.run_var.clone())
        self.y, self.out = _new((M, CH), dt), _new((M, CH), dt)
        self.mw = 3 if T <= 96 else (T + 31) // 32
        self.mask = _new((B * J * T * self.mw,), torch.int32, fill=-1) if mode == 1 else None
        self.stats = _new((_lib.GCN_STAT_WORDS,), torch.int64, fill=-1)
        self.coef = _new((256 * 8,), torch.float32)
        self.rc = lib.kasf_op_gcn_fwd(code, ptr(d["x_in"]), ptr(d["xn"]), ptr(d["uv"]), ptr(d["bn_w"]), ptr(d["bn_b"]), ptr(self.run_mean), ptr(self.run_var),
                                      ptr(d["ls1"]), ptr(self.y), ptr(self.mask), ptr(self.stats), ptr(self.coef), ptr(self.out), B, T, mode, k, int(training),
                                      MOMENTUM, stream())
        _lib.check(self.rc)
        torch.cuda.synchronize()
        # the operands as the kernels saw them, in fp64
        self.op = {n: _back(d[n]) for n in d}
        self.op["run_mean"], self.op["run_var"] = _back(self.run0[0][:nodes]), _back(self.run0[1][:nodes])

    def coef_rows(self):
        return _back(self.coef.view(256, 8)[:self.nodes, :4])

    def backward(self, g_dev):
        from kasportsformer_amd import _lib
        code, dt = DT[self.cd]
        self.r, self.duv = _new((self.M, CH), dt), _new((self.M, 2 * CH), dt)
        self.dls1, self.d_bn_w, self.d_bn_b = _new((CH,), torch.float32, 1.0), _new((256,), torch.float32, 1.0), _new((256,), torch.float32, 1.0)
        self.bstats = _new((_lib.GCN_STAT_WORDS,), torch.int64, fill=-1)
        _lib.check(self.lib.kasf_op_gcn_bwd(code, ptr(g_dev), ptr(self.d["xn"]), ptr(self.y), ptr(self.coef), ptr(self.mask), ptr(self.d["ls1"]), ptr(self.r),
                                            ptr(self.duv), ptr(self.dls1), ptr(self.d_bn_w), ptr(self.d_bn_b), ptr(self.bstats), self.B, self.T, self.mode,
                                            int(self.training), stream()))
        torch.cuda.synchronize()
        assert bool((self.d_bn_w[self.nodes:] == 1).all()) and bool((self.d_bn_b[self.nodes:] == 1).all()), "d_bn_w / d_bn_b written past the node count"
        return dict(r=_back(self.r), duv=_back(self.duv), dls1=_back(self.dls1) - 1, d_bn_w=_back(self.d_bn_w[:self.nodes]) - 1,
                    d_bn_b=_back(self.d_bn_b[:self.nodes]) - 1)


def _safe_g(inp_g, ref, cd, limit):
    """g with the elements of an undecidable ReLU gate zeroed (module docstring); rounded to the model dtype; returns (device tensor, fp64 copy, fraction zeroed)"""
    margin = ref.gate_margin()
    near = ref.flat(ref.z.abs() < margin)
    frac = float(near.double().mean())
    assert frac < limit, f"{frac:.2e} of the elements within {margin:.2e} of the ReLU gate: the inputs are degenerate"
    g_dev = _dev(torch.where(near, torch.zeros(()), inp_g), DT[cd][1])
    return g_dev, _back(g_dev), frac


def _check(name, got, want, bar, log):
    e = rel_err(got, want)
    log.append(f"{name} {e:.2e} (bar {bar:.2e})")
    return e < bar


def _fwd_bwd_parity(lib, cd, mode, T, B, k, training, inp=None, bars_fwd=None, extra_bar=None, gate_limit=1e-3, tag=""):
    """One forward + backward against the reference; returns the log lines (also printed).  extra_bar(name) widens an output's bar (test (d) only)."""
    inp = inp or _inputs(mode, T, B, k)
    run = Run(lib, cd, inp, mode, T, B, k, training)
    nodes, tol = run.nodes, TOL[cd]
    log, ok = [], True
    bar = lambda name, base=tol: base + (extra_bar(name) if extra_bar else 0.0)
    # ---- forward
    ref = Ref(run.op, mode, T, B, k, training, y_stored=_back(run.y))
    ok &= _check("y", _back(run.y), ref.flat(ref.y0), bar("y"), log)      # y0: the reference's own y, before the stored values are substituted
    if mode == 1:
        got = decode_masks(run.mask, B * J, T)
        want = ref.adj.bool()
        assert torch.equal(got, want), f"adjacency mask: {int((got != want).sum())} bits differ"
        deg = want.sum(-1)
        assert T <= k or bool((deg > k).any()), "no row with a tie at the k-th place: tie retention is not exercised"
        log.append(f"mask bit-equal, max degree {int(deg.max())} (k = {k})")
    ok &= _check("out", _back(run.out), ref.flat(ref.out_g), bar("out"), log)
    coef, coef_ref = run.coef_rows(), ref.coef()
    for c, name in enumerate(("scale", "shift", "mean", "rstd")):
        ok &= _check(f"coef.{name}", coef[:, c], coef_ref[:, c], bar("coef." + name), log)
    assert bool((run.run_mean[nodes:] == SENTINEL).all()) and bool((run.run_var[nodes:] == SENTINEL).all()), "running statistics written past the node count"
    if training:
        rm, rv = ref.running(MOMENTUM)
        ok &= _check("running_mean", _back(run.run_mean[:nodes]), rm, 1e-6 + (extra_bar("running") if extra_bar else 0.0), log)
        ok &= _check("running_var", _back(run.run_var[:nodes]), rv, 1e-6 + (extra_bar("running") if extra_bar else 0.0), log)
    else:
        assert torch.equal(run.run_mean, run.run0[0]) and torch.equal(run.run_var, run.run0[1]), "evaluation mode wrote the running statistics"
    # ---- backward
    g_dev, g, frac = _safe_g(inp["g"], ref, cd, gate_limit)
    got = run.backward(g_dev)
    hand = ref.backward_by_hand(g)
    want = ref.backward(g)
    for n in want:
        assert rel_err(hand[n], want[n]) < 1e-9, f"the hand-written BatchNorm backward disagrees with autograd on {n}"
    bars = {n: tol for n in want}
    if cd == "bf16":                                             # calibrated against the reference's own sensitivity to the kernels' bf16 storage points
        emu = ref.backward_by_hand(g, _round_bf16)
        bars = {n: max(tol, 2 * rel_err(emu[n], hand[n])) for n in want}
    for n in ("r", "duv", "dls1", "d_bn_w", "d_bn_b"):
        ok &= _check(n, got[n], want[n], bar(n, bars[n]), log)
    print(f"\n[gcn {tag}{cd} mode={mode} T={T} B={B} k={k} training={training}] gate-zeroed {frac:.1e}: " + "; ".join(log))
    assert ok, "; ".join(log)
    return run, ref


# ================================================================================================ (a) forward + backward parity
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("mode,T,B", PARITY_CASES)
def test_gcn_forward_backward(lib, cd, mode, T, B, training):
    """Every output of the two entries at the project's bars (fp32 1e-4; bf16 3e-2 forward, backward max(3e-2, 2 x the reference's own rounding sensitivity);
    that sensitivity is a property of the reference alone: 2e-3 .. 5e-3 at the shapes evaluated, so the bars print as 3.00e-02); the mask bit for bit; running
    statistics to 1e-6 (training) or untouched (evaluation).  Every figure and bar is printed."""
    _fwd_bwd_parity(lib, cd, mode, T, B, 4, training)


# ================================================================================================ (b) neighbour_num
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("T,B", [(27, 2), (100, 1)])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_gcn_neighbour_num(lib, cd, k, T, B):
    _fwd_bwd_parity(lib, cd, 1, T, B, k, 1)


# ================================================================================================ (c) exactness of the accumulator
def _decode_stats(words, nodes):
    """[4 slots][512][5] int64 -> per statistic the exact value (Fraction) and the poison word (slots added)"""
    w = words.cpu().numpy().reshape(4, 512, 5)
    assert not w[:, 2 * nodes:, :].any(), "statistics beyond the node count were written"
    tot, poison = [], []
    for i in range(2 * nodes):
        acc = 0
        for sl in range(4):
            for kk in range(4):
                acc += int(w[sl, i, kk]) << (52 * kk)            # units of 2^-110
        tot.append(Fraction(acc, 1 << 110))
        poison.append(int(sum(int(w[sl, i, 4]) for sl in range(4))))
    return tot, poison, w


FLOOR_UNIT = Fraction(1, 1 << 110)
MAX_WORKGROUPS = 1024           # "grids are capped at 1,024 workgroups" (k_gcn.hip): each floors at most once


# e: a unit exactly on a word boundary (2^-58); straddles of words 0|1, 1|2, 2|3; the top word (sum y^2 in units of 2^72 at e = 36).  e = -115 is this file's
# addition: units of y BELOW the accumulator's lowest bit, so that NEGATIVE partials lose bits and stat_add's floor correction decides the result.
@pytest.mark.parametrize("e", [-58, -40, -29, 0, 13, 36, -115])
@pytest.mark.parametrize("mode,T,B", [(0, 27, 43), (1, 27, 70)])      # 19,737 tokens: the capped 1,024-workgroup grid, all four slots; 1,190 tracks
def test_gcn_accumulator_is_exact(lib, mode, T, B, e):
    """fp32, V = 0, U = n 2^e with integers n in [-8, 8]: y reads back bit-equal to U, every fp32 partial sum is exact whatever the partition (per node sum n^2 <=
    64 x 152,320 < 2^24 units), so the totals are known exactly and the decoded words must EQUAL them -- except where units lie below 2^-110 (sum y^2 at
    e = -58, both sums at e = -115): there exact - 1024 x 2^-110 <= total <= exact (floor toward -inf, at most once per workgroup)."""
    M, nodes, count = B * T * J, (J if mode == 0 else T), _count(mode, B, T)
    gen = torch.Generator().manual_seed(77 + T + B)
    n = torch.randint(-8, 9, (M, CH), generator=gen)
    node_of = _ungroup(torch.arange(nodes).view(1, nodes, 1).expand(M // nodes, nodes, 1).contiguous(), mode, B, T).view(M)
    neg = torch.randint(-8, 0, (M, CH), generator=gen)
    n = torch.where((node_of == 3)[:, None] | (node_of == nodes - 1)[:, None], neg, n)      # two nodes with every n < 0
    U = torch.ldexp(n.float(), torch.tensor(e))
    assert torch.equal(torch.ldexp(U.double(), torch.tensor(-e)), n.double())
    inp = dict(_inputs(mode, T, B, 4))
    inp["uv"] = torch.cat([U, torch.zeros(M, CH)], dim=1)
    run = Run(lib, "fp32", inp, mode, T, B, 4, 1)
    assert torch.equal(run.y.cpu().view(torch.int32), U.view(torch.int32)), "y is not bit-equal to U"
    tot, poison, w = _decode_stats(run.stats, nodes)
    assert not any(poison), "poison word set"
    if mode == 0:
        assert all(w[sl].any() for sl in range(4)), "a slot copy stayed empty: the grid did not spread over the four slots"
    ng = _group(n, mode, B, T).numpy()                          # int64: the sums stay below 2^24
    s1 = [Fraction(int(ng[:, i, :].sum())) * Fraction(2) ** e for i in range(nodes)]
    s2 = [Fraction(int((ng[:, i, :] ** 2).sum())) * Fraction(2) ** (2 * e) for i in range(nodes)]
    assert max(int((ng[:, i, :] ** 2).sum()) for i in range(nodes)) < 2 ** 24
    slack = MAX_WORKGROUPS * FLOOR_UNIT
    for i in range(nodes):
        for which, exact, unit_exp in (("sum", s1[i], e), ("sum of squares", s2[i], 2 * e)):
            got = tot[2 * i + (which != "sum")]
            if unit_exp >= -110:
                assert got == exact, f"node {i} {which}: {float(got)!r} != {float(exact)!r} (difference {float(got - exact):.3e})"
            else:
                assert exact - slack <= got <= exact, f"node {i} {which}: total - exact = {float((got - exact) / FLOOR_UNIT)} units of 2^-110, outside [-1024, 0]"
    # coef follows from the sums (mean correctly rounded from the quotient; rstd = 1 / sqrt(var + 1e-5) in fp32); at e = -115 from the floored totals the kernel read
    coef = run.coef_rows()
    for i in range(nodes):
        a, b = (s1[i], s2[i]) if e >= -58 else (tot[2 * i], tot[2 * i + 1])
        mean = a / count
        var = max(b / count - mean * mean, Fraction(0))
        rstd = 1.0 / math.sqrt(float(var) + 1e-5)
        m_got, r_got = float(coef[i, 2]), float(coef[i, 3])
        assert abs(m_got - float(mean)) <= 1e-6 * abs(float(mean)), (i, m_got, float(mean))
        assert abs(r_got - rstd) <= 1e-6 * rstd, (i, r_got, rstd)


# ================================================================================================ (d) conditioning of the variance
def _conditioned_inputs(mode, T, B, rho):
    """U shifted per node so that |mean| / std of y is rho (sign alternating from node to node)"""
    inp = dict(_inputs(mode, T, B, 4))
    op = {n: inp[n].double() for n in inp}
    ref = Ref(op, mode, T, B, 4, 1)
    nodes = J if mode == 0 else T
    sign = torch.where(torch.arange(nodes) % 2 == 0, 1.0, -1.0).double()
    mu = sign * rho * ref.batch_var.sqrt() - ref.batch_mean
    uv = inp["uv"].clone()
    uv[:, :CH] += _ungroup(mu.view(1, nodes, 1).expand(B * T * J // nodes, nodes, 1).contiguous(), mode, B, T).float()
    inp["uv"] = uv
    return inp


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("mode,T,B", [(0, 27, 43), (1, 27, 70)])
def test_gcn_variance_conditioning_rho8(lib, cd, mode, T, B):
    """Every node at |mean| / std = 8: (a)'s bars, unchanged."""
    run, ref = _fwd_bwd_parity(lib, cd, mode, T, B, 4, 1, inp=_conditioned_inputs(mode, T, B, 8.0), tag="rho=8 ")
    rho = (ref.batch_mean.abs() / ref.batch_var.sqrt())
    assert 6.0 < float(rho.min()) and float(rho.max()) < 10.0, (float(rho.min()), float(rho.max()))


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("mode,T,B", [(0, 27, 43), (1, 27, 70)])
def test_gcn_variance_conditioning_rho64(lib, cd, mode, T, B):
    """Every node at |mean| / std = 64.  E[y^2] - mean^2 from fp32 per-workgroup partials loses (1 + rho^2) 2^-22 of the variance relative to a two-pass
    evaluation; the allowed error of an output is TOL[cd] plus twice the change of the fp64 reference's own output when its variance is multiplied by
    1 +- (1 + rho^2) 2^-22 (the sensitivities and the measured errors are printed)."""
    rho = 64.0
    delta = (1 + rho * rho) * 2.0 ** -22
    inp = _conditioned_inputs(mode, T, B, rho)
    sens = {}

    def extra(name):
        return 2 * sens.get(name, 0.0)

    # the reference's own sensitivity needs the stored y and the g the comparison uses: a first run supplies them (the same launches the comparison then repeats)
    probe = Run(lib, cd, inp, mode, T, B, 4, 1)
    y_st = _back(probe.y)
    base = Ref(probe.op, mode, T, B, 4, 1, y_stored=y_st)
    _, g, _ = _safe_g(inp["g"], base, cd, 0.05)
    base_out, base_coef, base_run = base.flat(base.out_g), base.coef(), base.running(MOMENTUM)
    base_grads = base.backward(g)
    for s in (1 + delta, 1 - delta):
        p = Ref(probe.op, mode, T, B, 4, 1, y_stored=y_st, var_scale=s)
        sens["out"] = max(sens.get("out", 0.0), rel_err(p.flat(p.out_g), base_out))
        for c, name in enumerate(("scale", "shift", "mean", "rstd")):
            sens["coef." + name] = max(sens.get("coef." + name, 0.0), rel_err(p.coef()[:, c], base_coef[:, c]))
        # the running variance is the batch variance itself: its sensitivity is delta x momentum-weighted share
        sens["running"] = max(sens.get("running", 0.0), rel_err((1 - MOMENTUM) * probe.op["run_var"] + MOMENTUM * s * base.batch_var * base.count / (base.count - 1), base_run[1]))
        for n, v in p.backward(g).items():
            sens[n] = max(sens.get(n, 0.0), rel_err(v, base_grads[n]))
    print(f"\n[gcn rho=64 {cd} mode={mode}] delta = {delta:.3e}; reference sensitivity: " + ", ".join(f"{n} {v:.2e}" for n, v in sorted(sens.items())))
    _fwd_bwd_parity(lib, cd, mode, T, B, 4, 1, inp=inp, extra_bar=extra, gate_limit=0.05, tag="rho=64 ")


# ================================================================================================ (e) non-finite input
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1])
def test_gcn_nonfinite_input_poisons_one_node(lib, cd, mode):
    """One +inf in one node's U: the call succeeds, that node's statistics are poisoned, its rows of `out` are NaN (as the reference's are: BatchNorm over a batch
    that holds an inf, then ReLU, which propagates NaN), every other node is unaffected."""
    T, B, k = 27, 2, 4
    nodes, bad = (J if mode == 0 else T), 5
    inp = dict(_inputs(mode, T, B, k))
    uv = inp["uv"].clone()
    tok = (1 * T + (3 if mode == 0 else bad)) * J + (bad if mode == 0 else 11)       # clip 1; spatial: frame 3, joint `bad`; temporal: frame `bad`, joint 11
    uv[tok, 40] = float("inf")
    inp["uv"] = uv
    run = Run(lib, cd, inp, mode, T, B, k, 1)
    assert run.rc == 0
    ref = Ref(run.op, mode, T, B, k, 1)
    out_ref, out = _group(ref.flat(ref.out_g), mode, B, T), _group(_back(run.out), mode, B, T)
    others = [i for i in range(nodes) if i != bad]
    assert bool(out_ref[:, bad].isnan().all()) and bool(out_ref[:, others].isfinite().all())
    assert bool(out[:, bad].isnan().all()), f"{int((~out[:, bad].isnan()).sum())} values of the poisoned node are not NaN"
    assert bool(out[:, others].isfinite().all())
    e = rel_err(out[:, others], out_ref[:, others])
    print(f"\n[gcn inf {cd} mode={mode}] other nodes' out {e:.2e}")
    assert e < TOL[cd]
    _, poison, _ = _decode_stats(run.stats, nodes)
    assert poison[2 * bad] != 0 and poison[2 * bad + 1] != 0
    assert not any(p for i, p in enumerate(poison) if i // 2 != bad)
