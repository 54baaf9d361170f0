"""The linear, data-gradient, weight-gradient and MLP kernels on their own (include/kasf.h: kasf_op_linear, kasf_op_linear_res, kasf_op_dgrad_lnbwd, kasf_op_dgrad_wg,
kasf_op_wgrad, kasf_op_wgrad_jobs, kasf_op_mlp_fwd, kasf_op_mlp_bwd, kasf_op_mlp_bwd_fused, kasf_op_cast) against fp64 torch math of the same operation on the dtype-rounded operands
(tests/dense_ref.py).  tests/test_gpu_ops.py keeps its own, older checks of the same entries.

How every comparison is set up:
  * Operands are built on the CPU from a fixed seed and rounded to the storage dtype (bf16; fp16 for w2 of the bf16 forward); the reference is fp64 on what the device
    holds.  Every operand that feeds a LayerNorm carries the planted rows of dense_ref.plant (constant, all-zero, variance 1e-6, mean 32, scale 1e3) in its first tile,
    its last (ragged) tile and the first tile of a workgroup's second walk.
  * Token-major operands have 64 rows of NaN behind row M: a kernel that reads a row >= M into a column sum (dgamma, dbeta, db1, gsum, dW) turns it into NaN.
  * Token-major outputs have 64 rows behind row M; written buffers start at the sentinel 7 and the tail must hold it bit for bit afterwards.  Accumulated buffers
    start at 1, scratch at NaN.  Every fixed-order case (scratch / partial) runs twice from identical inputs and must give the same bits.
  * Token-major outputs (y, xn_out, out, g_in, H, dZ) are judged PER ROW: the row's largest error over the row's own largest |ref|, the worst row (a constant row's
    LayerNorm backward is 316 x any other row).  Reductions are judged per tensor against their own largest value.  No pooling, no cosine, no floor.
  * Bars (dense_ref.BAR32, DIST16; none from a device run): fp32 mode bar32[op]; bf16 mode, stored outputs, per element |got - ref| <= 2^-8 |ref| + c[op] x row max,
    fp32 outputs c[op] x tensor max.  An accumulated output adds `adds x 2^-24 (1 + |ref|max) / |ref|max`: one addition on a fixed-order path, the launch's grid on the
    atomics (`_adds_*` restate the launchers).

Instantiations by test id (bf16 unless noted; fp32 mode runs the generic k_linear / k_linear_res / k_dgrad_lnbwd / k_wgrad / k_mlp_fwd / k_mlp_bwd <float>):
  test_linear           ln1-N384 / ln1-N256 / ln1-N128 -> k_linear_r<3 / 2 / 1, LN>;  ln0-N128 -> k_linear_r<1, false>;  ln0-N256 / ln0-N384 -> k_linear<bf16> (no persistent
                        instantiation: the fall-back);  N512-tanh -> k_linear<bf16, ..., ACT = 1> with and without LN
  test_linear_res       k_linear_r<1, false, RES> (fp32: k_linear_res<float>)
  test_dgrad_lnbwd      Kd384 / Kd128 (resid, xn) / Kd256 (accumulate, xn) / Kd256 (add, resid) -> k_dgrad_r<3 / 1 / 2 / 2>;  Kd512 and Kd128 (add, accumulate) -> k_dgrad_lnbwd<bf16>
  test_dgrad_wg         qkv / q / kv -> k_dgrad_r<3 / 1 / 2, ..., WG>;  uv_bias -> <2, ..., WG, BIAS>;  q_proj -> <1, ..., WG, false, PROJ>;  then k_wgrad_finish_jobs (reduction
                        role; proj job for q_proj) and k_col_finish
  test_wgrad            ln0 -> k_wgrad_ring<bf16> (fp32: k_wgrad<float, 1, false>);  ln1 -> k_wgrad<., ., true>;  partial given -> k_wgrad_reduce
  test_mlp_fwd          fp32 k_mlp_fwd<float>;  bf16 k_mlp_fwd_s with xn_out and with NULL (evaluation mode)
  test_mlp_bwd_wgrad    k_mlp_bwd<float> / k_mlp_bwd<bf16> + the two kasf_op_wgrad launches of the fp32 mode's path
  test_mlp_bwd_fused    k_mlp_bwd_s<false> + k_lnbwd_sum4_fin<2> (fin blocks: mlp_wfinish_body)
  test_wgrad_jobs       k_wgrad_ring_jobs (wgrad_ring_body<bf16, BF16P>) + k_wgrad_finish_jobs:  att2 / bone3 -> two / three streaming jobs, job 0 finished with the
                        layer-scale algebra;  att1_red / one_red2 -> the reduction role beside the jobs;  ext_self / ext_bone -> the ext job (tiles and rows from
                        another kernel) beside one / two streaming jobs.  M 769 / 2049 / 4097 / 6209: the remainder branch of the XCD order (splits % 8 != 0)
"""
import ctypes as C

import pytest
import torch

from tests import dense_ref as R
from tests.gpu_util import DT, ptr, stream

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
PAD = 64
CDS = ["fp32", "bf16"]
F64 = torch.float64


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


def _dev(t, dtype=torch.float32):
    d = t.to(dtype).cuda().contiguous()
    _KEEP.append(d)
    return d


def _rows_in(t, dtype):
    """a token-major operand [M,C] on the device with PAD rows of NaN behind it"""
    d = torch.full((t.shape[0] + PAD, t.shape[1]), float("nan"), dtype=dtype)
    d[:t.shape[0]] = t.to(dtype)
    return _dev(d, dtype)


def _new(shape, dtype=torch.float32, fill=SENTINEL):
    d = torch.full(shape if isinstance(shape, tuple) else (shape,), fill, device="cuda", dtype=dtype)
    _KEEP.append(d)
    return d


def _rows_out(M, C, dtype, init=None):
    """a token-major output [M + PAD, C] holding the sentinel (rows < M: `init` where the op accumulates into it)"""
    d = _new((M + PAD, C), dtype)
    if init is not None:
        d[:M] = init.to(dtype).cuda()
    return d


def _back(t):
    return t.detach().double().cpu()


def _ok(rc, lib):
    assert rc == 0, (rc, lib.kasf_last_error())
    torch.cuda.synchronize()


def _tail_kept(buf, M, what):
    assert bool((buf[M:] == SENTINEL).all()), f"{what}: rows >= M were written"


def _all_nan(buf, what):
    assert bool(torch.isnan(buf).all()), f"{what}: the guard behind the scratch was written"


def _same_bits(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs between two runs from identical inputs"


class Log:
    def __init__(self, tag, cd, op):
        self.tag, self.cd, self.op, self.lines, self.ok = tag, cd, op, [], True
        self.bar = R.BAR32[op] if cd == "fp32" else R.c16(op)

    def rows(self, name, got, ref, no16=False):
        """a token-major output stored in the model dtype, per row; no16: no 16-bit point lies in front of this output (xn_out: its own rounding is the ulp term), so
        its bf16 distance is 0 and its c is the fp32 bar"""
        bar = R.BAR32[self.op] if no16 else self.bar
        if self.cd == "fp32":
            e, row = R.row_err(got, ref)
            self.lines.append(f"{name} {e:.2e} at row {row} (bar {bar:.2e})")
        else:
            e, row = R.row_excess(got, ref)
            self.lines.append(f"{name} excess over a bf16 ulp {e:.2e} at row {row} (bar {bar:.2e})")
        self.ok &= e <= bar
        return e

    def red(self, name, got, ref, adds=0, no16=False):
        """an fp32 reduction, per tensor; adds: fp32 additions into the buffer (holding 1) that it was accumulated into; no16: a plain column sum of an operand
        (dbias, gsum, dproj_b): no 16-bit point, the fp32 bar in both modes"""
        mx = max(float(ref.abs().max()), 1e-300)
        bar = (R.BAR32[self.op] if no16 else self.bar) + adds * 2.0 ** -24 * (1 + mx) / mx
        e = R.rel_err(got, ref)
        self.lines.append(f"{name} {e:.2e} (bar {bar:.2e})")
        self.ok &= e <= bar
        return e

    def done(self):
        print(f"\n[dense {self.tag}] " + "; ".join(self.lines))
        assert self.ok, f"{self.tag}: " + "; ".join(self.lines)


def _f64(ops, names):
    return [ops[n].to(F64) if ops[n] is not None else None for n in names]


def _exact_rows(xn_dev, where, beta, cd, what):
    """LN of a constant or all-zero row is beta exactly (fp32), the bf16 rounding of beta (bf16): sums of 128 equal values of <= 8 significant bits are exact in fp32"""
    want = beta.to(DT[cd][1])
    got = xn_dev.cpu()
    for r in where.get("const", []) + where.get("zero", []):
        assert torch.equal(got[r], want), f"{what}: LN of the planted constant row {r} is not beta exactly"


# ================================================================================================ linear
def _linear_case(cd, use_ln, N, act, M):
    i = R.stored(R.linear_inputs(use_ln, N, act, M), cd)
    return i, R.linear_ref(*_f64(i, ("a", "w", "bias", "g", "b")), act)


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("use_ln,N,act", R.LINEAR_CASES, ids=[f"ln{c[0]}-N{c[1]}" + ("-tanh" if c[2] else "") for c in R.LINEAR_CASES])
@pytest.mark.parametrize("M", R.LINEAR_M)
def test_linear(lib, cd, use_ln, N, act, M):
    code, dt = DT[cd]
    i, ref = _linear_case(cd, use_ln, N, act, M)
    a, w, bias = _rows_in(i["a"], dt), _dev(i["w"], dt), _dev(i["bias"])
    g, b = (_dev(i["g"]), _dev(i["b"])) if use_ln else (None, None)
    log = Log(f"linear {cd} ln={use_ln} N={N} act={act} M={M}", cd, "linear_tanh" if act else "linear")
    ys = []
    for want_xn in ((True, False) if use_ln else (False,)):
        y, xn = _rows_out(M, N, dt), _rows_out(M, 128, dt)
        _ok(lib.kasf_op_linear(code, ptr(a), ptr(w), ptr(bias), ptr(y), M, N, ptr(g), ptr(b), ptr(xn) if want_xn else None, act, stream()), lib)
        _tail_kept(y, M, log.tag + " y")
        log.rows(f"y[xn_out={int(want_xn)}]", _back(y[:M]), ref["y"])
        if want_xn:
            _tail_kept(xn, M, log.tag + " xn_out")
            log.rows("xn_out", _back(xn[:M]), ref["xn"], no16=True)
            _exact_rows(xn[:M], i["where"], i["b"], cd, log.tag)
        else:
            assert bool((xn == SENTINEL).all())
        if act:                                            # |z| > 20: tanh is +-1 exactly in the reference's rounding to fp32, and must be on the device
            sat = ref["z"].abs() > 20
            assert int(sat.sum()) >= 2 * M and torch.equal(y[:M].cpu().double()[sat], torch.sign(ref["z"][sat])), f"{log.tag}: tanh of |z| > 20 is not +-1 exactly"
        ys.append(y[:M].clone())
    if len(ys) == 2:
        assert torch.equal(ys[0], ys[1]), f"{log.tag}: y differs between xn_out present and NULL"
    log.done()


def _linear_res_case(cd, M):
    i = R.stored(R.linear_res_inputs(M), cd)
    return i, R.linear_res_ref(*_f64(i, ("a", "w", "bias", "ls", "resid")))


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("M", R.LINEAR_M)
def test_linear_res(lib, cd, M):
    code, dt = DT[cd]
    i, ref = _linear_res_case(cd, M)
    a, resid, w = _rows_in(i["a"], dt), _rows_in(i["resid"], dt), _dev(i["w"], dt)
    out = _rows_out(M, 128, dt)
    _ok(lib.kasf_op_linear_res(code, ptr(a), ptr(w), ptr(_dev(i["bias"])), ptr(_dev(i["ls"])), ptr(resid), ptr(out), M, stream()), lib)
    _tail_kept(out, M, "linear_res out")
    log = Log(f"linear_res {cd} M={M}", cd, "linear_res")
    log.rows("out", _back(out[:M]), ref["out"])
    log.done()


# ================================================================================================ data gradient + LayerNorm backward
def _dgrad_sel(i, use_add, use_resid, acc, dt=F64):
    return [i[k].to(dt) if use else None for k, use in (("dy", 1), ("wt", 1), ("add", use_add), ("x", 1), ("g", 1), ("resid", use_resid), ("prev", acc), ("b", 1))]


def _dgrad_case(cd, Kd, use_add, use_resid, acc, M):
    i = R.stored(R.dgrad_inputs(Kd, M), cd)
    return i, R.dgrad_ref(*_dgrad_sel(i, use_add, use_resid, acc))


def _adds_dgrad(cd, Kd, use_add, use_resid, acc, want_xn, M):
    """kasf_op_dgrad_lnbwd has no column sink: one atomicAdd per workgroup into dgamma / dbeta.  bf16, the four persistent instantiations: the workgroups that own a
    tile (launch_dgrad_r); otherwise k_dgrad_lnbwd's grid of 64-row tiles."""
    persistent = cd == "bf16" and (Kd, use_add, use_resid, acc, want_xn) in ((384, False, True, False, True), (128, False, True, False, True),
                                                                             (256, False, False, True, True), (256, True, True, False, False))
    return len(R.wg_ranges(M)) if persistent else (M + 63) // 64


def _dgrad_operands(i, dt, use_add, use_resid):
    return dict(dy=_rows_in(i["dy"], dt), x=_rows_in(i["x"], dt), wt=_dev(i["wt"], dt), add=_rows_in(i["add"], dt) if use_add else None,
                resid=_rows_in(i["resid"], dt) if use_resid else None, g=_dev(i["g"]), b=_dev(i["b"]))


def _run_dgrad(lib, cd, i, d, Kd, acc, want_xn, M):
    code, dt = DT[cd]
    out = _rows_out(M, 128, dt, i["prev"] if acc else None)
    xn = _rows_out(M, 128, dt)
    dg, db = _new(128, fill=1.0), _new(128, fill=1.0)
    _ok(lib.kasf_op_dgrad_lnbwd(code, ptr(d["dy"]), Kd, ptr(d["wt"]), ptr(d["add"]), ptr(d["x"]), ptr(d["g"]), ptr(d["resid"]), ptr(out), int(acc), ptr(dg), ptr(db), M,
                                ptr(xn) if want_xn else None, ptr(d["b"]) if want_xn else None, stream()), lib)
    return dict(out=out, xn=xn, dgamma=dg, dbeta=db)


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("Kd,use_add,use_resid,acc,want_xn", R.DGRAD_CASES, ids=[f"Kd{c[0]}-add{int(c[1])}-resid{int(c[2])}-acc{int(c[3])}-xn{int(c[4])}" for c in R.DGRAD_CASES])
@pytest.mark.parametrize("M", R.DGRAD_M)
def test_dgrad_lnbwd(lib, cd, Kd, use_add, use_resid, acc, want_xn, M):
    i, ref = _dgrad_case(cd, Kd, use_add, use_resid, acc, M)
    d = _dgrad_operands(i, DT[cd][1], use_add, use_resid)
    got = _run_dgrad(lib, cd, i, d, Kd, acc, want_xn, M)
    log = Log(f"dgrad_lnbwd {cd} Kd={Kd} add={use_add} resid={use_resid} acc={acc} xn={want_xn} M={M}", cd, "dgrad")
    _tail_kept(got["out"], M, log.tag + " out")
    _tail_kept(got["xn"], M, log.tag + " xn_out")
    log.rows("out", _back(got["out"][:M]), ref["out"])
    adds = _adds_dgrad(cd, Kd, use_add, use_resid, acc, want_xn, M)
    log.red("dgamma", _back(got["dgamma"]) - 1, ref["dgamma"], adds)
    log.red("dbeta", _back(got["dbeta"]) - 1, ref["dbeta"], adds)
    if want_xn:
        log.rows("xn_out", _back(got["xn"][:M]), ref["xn"], no16=True)
        _exact_rows(got["xn"][:M], i["where"], i["b"], cd, log.tag)
    else:
        assert bool((got["xn"] == SENTINEL).all())
    log.done()


# ================================================================================================ fused data + weight gradient (bf16)
def _wg_case(form, M):
    Kd, use_resid, acc, bias, proj = R.WG_FORMS[form]
    i = R.stored(R.dgrad_inputs(Kd, M, proj), "bf16")
    sel = _dgrad_sel(i, bias, use_resid, acc) + [bias] + [i[k].to(F64) if proj else None for k in ("o", "pw", "pb", "pls")]
    return i, R.dgrad_wg_ref(*sel)


WPROJ_BYTES = 256 * 128 * 128 * 2 + 256 * 128 * 4


def _run_dgrad_wg(lib, i, d, form, M):
    Kd, use_resid, acc, bias, proj = R.WG_FORMS[form]
    bf = torch.bfloat16
    out = _rows_out(M, 128, bf, i["prev"] if acc else None)
    one = lambda *s: _new(tuple(s), fill=1.0)
    r = dict(out=out, dgamma=one(128), dbeta=one(128), dw=one(Kd, 128), dbias=one(Kd), dproj_w=one(128, 128), dproj_b=one(128), dproj_ls=one(128))
    rows = len(R.wg_ranges(M))
    need = (rows * (512 if bias else 256) + 63) // 64 * 64
    scratch = _new(need + 64, fill=float("nan"))
    wpart = _new(256 * Kd * 128 + 64, bf, float("nan"))
    ppart = _new(WPROJ_BYTES // 2 + 64, bf, float("nan")) if proj else None
    pj = lambda t: ptr(t) if proj else None
    rc = lib.kasf_op_dgrad_wg(ptr(d["dy"]), Kd, ptr(d["wt"]), ptr(d["add"]) if bias else None, ptr(d["x"]), ptr(d["g"]), ptr(d["b"]), ptr(d["resid"]), ptr(out), int(acc),
                              ptr(r["dgamma"]), ptr(r["dbeta"]), ptr(r["dw"]), ptr(r["dbias"]) if bias else None, pj(d.get("o")), pj(d.get("pw")), pj(d.get("pb")),
                              pj(d.get("pls")), pj(r["dproj_w"]), pj(r["dproj_b"]), pj(r["dproj_ls"]), M, ptr(wpart), 256 * Kd * 128 * 2, ptr(ppart), WPROJ_BYTES if proj else 0,
                              ptr(scratch), need, stream())
    _ok(rc, lib)
    _all_nan(scratch[need:], "dgrad_wg scratch")
    _all_nan(wpart[256 * Kd * 128:], "dgrad_wg wpart")
    if proj:
        _all_nan(ppart[WPROJ_BYTES // 2:], "dgrad_wg proj_part")
    return r


@pytest.mark.parametrize("form", list(R.WG_FORMS))
@pytest.mark.parametrize("M", R.DGRAD_WG_M)
def test_dgrad_wg(lib, form, M):
    Kd, use_resid, acc, bias, proj = R.WG_FORMS[form]
    bf = torch.bfloat16
    i, ref = _wg_case(form, M)
    d = _dgrad_operands(i, bf, bias, use_resid)
    if proj:
        d.update(o=_rows_in(i["o"], bf), pw=_dev(i["pw"]), pb=_dev(i["pb"]), pls=_dev(i["pls"]))
    got = _run_dgrad_wg(lib, i, d, form, M)
    log = Log(f"dgrad_wg {form} M={M}", "bf16", "dgrad_wg")
    _tail_kept(got["out"], M, log.tag + " out")
    log.rows("out", _back(got["out"][:M]), ref["out"])
    names = ["dgamma", "dbeta", "dw"] + (["dbias"] if bias else []) + (["dproj_w", "dproj_b", "dproj_ls"] if proj else [])
    for n in names:
        log.red(n, _back(got[n]) - 1, ref[n], 1, no16=n in ("dbias", "dproj_b"))
    for n in set(got) - set(names) - {"out"}:
        assert bool((got[n] == 1).all()), f"{log.tag}: {n} is not part of this form"
    # fixed order throughout: the same bits from a second run
    again = _run_dgrad_wg(lib, i, d, form, M)
    _same_bits({n: got[n] for n in names + ["out"]}, again, log.tag)
    # the data gradient is the non-fused kernel's arithmetic: the same bits in `out` (kasf_op_dgrad_lnbwd runs k_dgrad_r of the same KC / RESID / ADD / ACC; uv_bias: its
    # XN = false form).  dgamma / dbeta meet there by atomics, one per workgroup: the same bits only where one workgroup owns every tile
    plain = _run_dgrad(lib, "bf16", i, d, Kd, acc, not bias, M)
    assert torch.equal(plain["out"], got["out"]), f"{log.tag}: out differs from kasf_op_dgrad_lnbwd"
    if len(R.wg_ranges(M)) == 1:
        assert torch.equal(plain["dgamma"], got["dgamma"]) and torch.equal(plain["dbeta"], got["dbeta"]), f"{log.tag}: dgamma / dbeta differ from kasf_op_dgrad_lnbwd"
    # dw against kasf_op_wgrad on the same operands (fp32 partial tiles there, one bf16 partial tile per workgroup here)
    dw2, db2 = _new((Kd, 128), fill=1.0), _new(Kd, fill=1.0)
    _ok(lib.kasf_op_wgrad(1, ptr(d["dy"]), Kd, ptr(d["x"]), 128, ptr(d["g"]), ptr(d["b"]), ptr(dw2), ptr(db2), M, None, 0, stream()), lib)
    log.red("dw against kasf_op_wgrad", _back(got["dw"]) - 1, _back(dw2) - 1, 1 + R.wgrad_splits(Kd, 128, M)[0])
    if bias:
        log.red("dbias against kasf_op_wgrad", _back(got["dbias"]) - 1, _back(db2) - 1, 1 + R.wgrad_splits(Kd, 128, M)[0], no16=True)
    log.done()


def test_dgrad_wg_refuses_short_scratch(lib):
    """sizes below what kasf_dgrad_wg_supported and the sink need are error 2 before a launch: every buffer keeps its start value"""
    M, form = 8193, "q"
    i, _ = _wg_case(form, M)
    d = _dgrad_operands(i, torch.bfloat16, False, True)
    out, dg, db, dw = _rows_out(M, 128, torch.bfloat16), _new(128, fill=1.0), _new(128, fill=1.0), _new((128, 128), fill=1.0)
    wpart, scratch = _new(256 * 128 * 128, torch.bfloat16, float("nan")), _new(129 * 256, fill=float("nan"))
    call = lambda wbytes, sfloats: lib.kasf_op_dgrad_wg(ptr(d["dy"]), 128, ptr(d["wt"]), None, ptr(d["x"]), ptr(d["g"]), ptr(d["b"]), ptr(d["resid"]), ptr(out), 0, ptr(dg),
                                                        ptr(db), ptr(dw), None, None, None, None, None, None, None, None, M, ptr(wpart), wbytes, None, 0, ptr(scratch),
                                                        sfloats, stream())
    assert call(256 * 128 * 128 * 2 - 2, 129 * 256) == 2 and b"wpart_bytes" in lib.kasf_last_error()
    assert call(256 * 128 * 128 * 2, 129 * 256 - 64) == 2 and b"scratch_floats" in lib.kasf_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((dw == 1).all()) and bool((dg == 1).all()) and bool(torch.isnan(wpart).all()) and bool(torch.isnan(scratch).all())
    _ok(call(256 * 128 * 128 * 2, 129 * 256), lib)
    assert not bool((dw == 1).all())


# ================================================================================================ weight gradient
def _wgrad_case(cd, N, K, use_ln, M):
    i = R.stored(R.wgrad_inputs(N, K, use_ln, M), cd)
    return i, R.wgrad_ref(*_f64(i, ("g", "x", "gm", "bt")))


WGRAD_CASES = [(N, K, ln) for N, K in R.WGRAD_NK for ln in ((1, 0) if K == 128 else (0,))]


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("N,K,use_ln", WGRAD_CASES, ids=[f"N{c[0]}-K{c[1]}-ln{c[2]}" for c in WGRAD_CASES])
@pytest.mark.parametrize("M", R.WGRAD_M)
def test_wgrad(lib, cd, N, K, use_ln, M):
    code, dt = DT[cd]
    i, ref = _wgrad_case(cd, N, K, use_ln, M)
    g, x = _rows_in(i["g"], dt), _rows_in(i["x"], dt)
    gm, bt = (_dev(i["gm"]), _dev(i["bt"])) if use_ln else (None, None)
    splits, need = R.wgrad_splits(N, K, M)
    log = Log(f"wgrad {cd} N={N} K={K} ln={use_ln} M={M} splits={splits}", cd, "wgrad")

    def run(form):
        dw, dbias = _new((N, K), fill=1.0), _new(N, fill=1.0)
        part = _new(need + 64, fill=float("nan")) if form != "null" else None
        floats = {"exact": need, "null": 0, "short": need - 1}[form]
        _ok(lib.kasf_op_wgrad(code, ptr(g), N, ptr(x), K, ptr(gm), ptr(bt), ptr(dw), ptr(dbias), M, ptr(part), floats, stream()), lib)
        if form == "exact":
            _all_nan(part[need:], log.tag + " partial")
        if form == "short":
            _all_nan(part, log.tag + " partial (too small: the launch must fall back to the atomics and leave it alone)")
        return dict(dw=dw, dbias=dbias)

    for form in ("exact", "null", "short"):                 # partial given and large enough (fixed order) / NULL / given but one float short (both: fp32 atomics)
        got = run(form)
        adds = 1 if form == "exact" else splits
        log.red(f"dw[{form}]", _back(got["dw"]) - 1, ref["dw"], adds)
        log.red(f"dbias[{form}]", _back(got["dbias"]) - 1, ref["dbias"], adds, no16=True)
        if form == "exact":
            _same_bits(got, run(form), log.tag)
    log.done()


# ================================================================================================ several weight gradients in one launch (bf16)
def _parr(ts):
    """a host array of device pointers (NULL for None); the tensors stay alive in _KEEP"""
    a = (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() if t is not None else None for t in ts])
    _KEEP.append(a)
    return C.c_void_p(C.addressof(a))


def _parts_in(t):
    """bf16 partial tiles [parts, ...] (a reduction's, the ext job's) with one part of NaN behind them: a loop that runs one part too far sums it"""
    d = torch.full((t.shape[0] + 1, *t.shape[1:]), float("nan"), dtype=torch.bfloat16)
    d[:t.shape[0]] = t.to(torch.bfloat16)
    return _dev(d, torch.bfloat16)


def _jobs_operands(i):
    bf = torch.bfloat16
    d = dict(G=[_rows_in(t, bf) for t in i["G"]], X=[_rows_in(t, bf) for t in i["X"]], W=_dev(i["W"]), bias=_dev(i["bias"]), ls=_dev(i["ls"]),
             red=[_parts_in(t) for t in i["red"]], ext_part=None, ext_brow=None)
    if i["ext_part"] is not None:
        d["ext_part"] = _parts_in(i["ext_part"])
        d["ext_brow"] = _dev(torch.cat([i["ext_brow"], torch.full((1, 128), float("nan"))]))
    return d


def _run_jobs(lib, i, d, M, floats=None):
    """-> (return code, {output: the accumulated buffer (started at 1)}, partial, the floats the launcher needs)"""
    Ns, fin_job = i["Ns"], i["fin_job"]
    one = lambda *s: _new(tuple(s), fill=1.0)
    r = {f"dw{j}": one(N, 128) for j, N in enumerate(Ns)}
    r.update({f"red{k}": one(t.shape[1]) for k, t in enumerate(i["red"])})
    ext = d["ext_part"] is not None
    if fin_job >= 0 or ext:
        r.update(db=one(128), dls=one(128))
    if ext:
        r["ext_dw"] = one(128, 128)
    need = R.jobs_partial_floats(M, Ns, fin_job)
    part = _new(need + 64, fill=float("nan"))
    dbias = [r["db"] if j == fin_job else None for j in range(len(Ns))]
    fin = (lambda t: ptr(t)) if fin_job >= 0 or ext else (lambda t: None)
    nparts = (C.c_int32 * 2)(*[t.shape[0] for t in i["red"]])
    elems = (C.c_int32 * 2)(*[t.shape[1] for t in i["red"]])
    _KEEP.extend([nparts, elems])
    nred = len(i["red"])
    rc = lib.kasf_op_wgrad_jobs(len(Ns), _parr(d["G"]), _parr(d["X"]), _parr_i32(Ns), _parr([r[f"dw{j}"] for j in range(len(Ns))]), _parr(dbias), fin_job, fin(d["W"]),
                                fin(d["bias"]), fin(d["ls"]), fin(r.get("dls")), M, ptr(part), need if floats is None else floats, nred,
                                _parr(d["red"]) if nred else None, _parr([r[f"red{k}"] for k in range(nred)]) if nred else None,
                                C.c_void_p(C.addressof(nparts)) if nred else None, C.c_void_p(C.addressof(elems)) if nred else None, ptr(d["ext_part"]),
                                ptr(d["ext_brow"]), i["ext_part"].shape[0] if ext else 0, ptr(r.get("ext_dw")), ptr(r["db"]) if ext else None, stream())
    if ext:
        r["ext_db"] = r.pop("db")
    return rc, r, part, need


def _parr_i32(v):
    a = (C.c_int32 * len(v))(*v)
    _KEEP.append(a)
    return C.c_void_p(C.addressof(a))


JOBS_CASES = [(mix, M, parts) for mix in R.JOBS_MIXES for M, parts in R.jobs_cases(mix)]


@pytest.mark.parametrize("mix,M,parts", JOBS_CASES, ids=[f"{c[0]}-M{c[1]}-parts{c[2]}" for c in JOBS_CASES])
def test_wgrad_jobs(lib, mix, M, parts):
    """kasf_launch_wgrad_jobs as block_backward launches it: every job's dW, the fin job's layer-scale algebra, the reductions riding in the finish launch and the ext
    job, each per tensor against fp64 on the bf16 operands; one bf16 partial tile per job and split is the 16-bit point (dense_ref.wgrad_jobs_ref)"""
    i = R.jobs_inputs(mix, M, parts)
    ref = R.wgrad_jobs_ref(*R.jobs_sel(i, F64))
    d = _jobs_operands(i)
    splits, sl = R.jobs_splits(M, i["Ns"])
    log = Log(f"wgrad_jobs {mix} M={M} parts={parts} splits={splits} slice={sl}", "bf16", "wgrad_jobs")
    rc, got, part, need = _run_jobs(lib, i, d, M)
    _ok(rc, lib)
    _all_nan(part[need:], log.tag + " partial")
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for n in sorted(ref):
        log.red(n, _back(got[n]) - 1, ref[n], 1, no16=R.jobs_no16(n, i))
    rc, again, part, _ = _run_jobs(lib, i, d, M)
    _ok(rc, lib)
    _same_bits(got, again, log.tag)
    log.done()


def test_wgrad_jobs_refuses_short_scratch(lib):
    """one float below what the launcher asks is error 2 before a launch: every buffer keeps its start value"""
    mix, M = "att2", 2049
    i = R.jobs_inputs(mix, M, 0)
    d = _jobs_operands(i)
    need = R.jobs_partial_floats(M, i["Ns"], i["fin_job"])
    rc, got, part, _ = _run_jobs(lib, i, d, M, floats=need - 1)
    assert rc == 2 and b"partial_floats" in lib.kasf_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in got.values()) and bool(torch.isnan(part).all())
    rc, got, part, _ = _run_jobs(lib, i, d, M, floats=need)
    _ok(rc, lib)
    assert not any(bool((t == 1).all()) for t in got.values())


def test_wgrad_jobs_isolation(lib):
    """job 1's operands redrawn: job 0's dW, db and dls keep their bits (a job reads and writes its own tiles and rows only)"""
    mix, M = "att2", 2049
    a, b = R.jobs_inputs(mix, M, 0), R.jobs_inputs(mix, M, 0, 1)
    rc, ga, _, _ = _run_jobs(lib, a, _jobs_operands(a), M)
    _ok(rc, lib)
    rc, gb, _, _ = _run_jobs(lib, b, _jobs_operands(b), M)
    _ok(rc, lib)
    _same_bits({n: ga[n] for n in ("dw0", "db", "dls")}, gb, "wgrad_jobs isolation")
    assert not torch.equal(ga["dw1"], gb["dw1"])


# ================================================================================================ MLP
def _mlp_fwd_case(cd, M):
    i = R.stored(R.mlp_inputs(M), cd, f16=("W2",))
    return i, R.mlp_fwd_ref(*_f64(i, ("x", "gm", "bt", "W1", "b1", "W2", "b2", "ls")))


def _mlp_params_dev(i, dt, fwd):
    d = dict(gm=_dev(i["gm"]), bt=_dev(i["bt"]), W1=_dev(i["W1"], dt), b1=_dev(i["b1"]), b2=_dev(i["b2"]), ls=_dev(i["ls"]))
    if fwd:
        d["W2"] = _dev(i["W2"], torch.float16 if dt == torch.bfloat16 else dt)      # bf16 mode: GEMM2 runs on fp16 operands (kasf.h)
    else:
        d["W2ts"], d["W1t"] = _dev(i["W2s"].T.contiguous(), dt), _dev(i["W1"].T.contiguous(), dt)      # [512,128] layer-scaled, [128,512]
    return d


@pytest.mark.parametrize("cd,M", [(cd, M) for cd in CDS for M in R.MLP_FWD_M[cd]])
def test_mlp_fwd(lib, cd, M):
    code, dt = DT[cd]
    i, ref = _mlp_fwd_case(cd, M)
    x, p = _rows_in(i["x"], dt), _mlp_params_dev(i, dt, True)
    log = Log(f"mlp_fwd {cd} M={M}", cd, "mlp_fwd")
    if M >= 459:
        assert float(ref["z"].max()) > 12 and float(ref["z"].min()) < -12, "the planted hidden units do not reach +-12"
    outs = []
    for want_xn in ((True, False) if cd == "bf16" else (False,)):
        out, xn = _rows_out(M, 128, dt), _rows_out(M, 128, dt)
        _ok(lib.kasf_op_mlp_fwd(code, ptr(x), ptr(p["gm"]), ptr(p["bt"]), ptr(p["W1"]), ptr(p["b1"]), ptr(p["W2"]), ptr(p["b2"]), ptr(p["ls"]), ptr(out), M,
                                ptr(xn) if want_xn else None, stream()), lib)
        _tail_kept(out, M, log.tag + " out")
        _tail_kept(xn, M, log.tag + " xn_out")
        log.rows(f"out[xn_out={int(want_xn)}]", _back(out[:M]), ref["out"])
        if want_xn:
            log.rows("xn_out", _back(xn[:M]), ref["xn"], no16=True)
            _exact_rows(xn[:M], i["where"], i["bt"], cd, log.tag)
        else:
            assert bool((xn == SENTINEL).all())
        outs.append(out[:M].clone())
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), f"{log.tag}: out differs between training (xn_out) and evaluation (NULL) form"
    log.done()


def _mlp_bwd_case(cd, M):
    i = R.stored(R.mlp_inputs(M), cd)
    return i, R.mlp_bwd_ref(*_f64(i, ("x", "gout", "gm", "bt", "W1", "b1", "W2s")))


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("M", R.MLP_BWD_M)
def test_mlp_bwd_wgrad(lib, cd, M):
    """kasf_op_mlp_bwd + the two kasf_op_wgrad launches (the fp32 mode's path; bf16: the generic kernels)"""
    code, dt = DT[cd]
    i, ref = _mlp_bwd_case(cd, M)
    x, gout, p = _rows_in(i["x"], dt), _rows_in(i["gout"], dt), _mlp_params_dev(i, dt, False)
    H, dZ, gin = _rows_out(M, 512, dt), _rows_out(M, 512, dt), _rows_out(M, 128, dt)
    one = lambda *s: _new(tuple(s), fill=1.0)
    dg, db, dW1, db1, dW2, gsum = one(128), one(128), one(512, 128), one(512), one(128, 512), one(128)
    _ok(lib.kasf_op_mlp_bwd(code, ptr(x), ptr(gout), ptr(p["gm"]), ptr(p["bt"]), ptr(p["W1"]), ptr(p["b1"]), ptr(p["W2ts"]), ptr(p["W1t"]), ptr(H), ptr(dZ), ptr(gin),
                            ptr(dg), ptr(db), M, stream()), lib)
    log = Log(f"mlp_bwd {cd} M={M}", cd, "mlp_bwd")
    for n, buf in (("H", H), ("dZ", dZ), ("g_in", gin)):
        _tail_kept(buf, M, f"{log.tag} {n}")
        log.rows(n, _back(buf[:M]), ref[n])
    adds = (M + (63 if cd == "bf16" else 31)) // (64 if cd == "bf16" else 32)          # k_mlp_bwd's grid: one atomicAdd per workgroup without a sink
    log.red("dgamma", _back(dg) - 1, ref["dgamma"], adds)
    log.red("dbeta", _back(db) - 1, ref["dbeta"], adds)
    # the weight gradients from what the kernel stored: dW1 = dZ^T LN(x) (atomics), dW2 unscaled = g^T H with gsum = colsum(g) (split partials + k_wgrad_reduce)
    dZ[M:], H[M:] = float("nan"), float("nan")
    s1, s2 = R.wgrad_splits(512, 128, M)[0], R.wgrad_splits(128, 512, M)
    part = _new(s2[1], fill=float("nan"))
    _ok(lib.kasf_op_wgrad(code, ptr(dZ), 512, ptr(x), 128, ptr(p["gm"]), ptr(p["bt"]), ptr(dW1), ptr(db1), M, None, 0, stream()), lib)
    _ok(lib.kasf_op_wgrad(code, ptr(gout), 128, ptr(H), 512, None, None, ptr(dW2), ptr(gsum), M, ptr(part), s2[1], stream()), lib)
    log.red("dW1", _back(dW1) - 1, ref["dW1"], s1)
    log.red("db1", _back(db1) - 1, ref["db1"], s1)
    log.red("dW2 unscaled", _back(dW2) - 1, ref["dW2u"], 1)
    log.red("gsum", _back(gsum) - 1, ref["gsum"], 1, no16=True)
    log.done()


@pytest.mark.parametrize("M", R.MLP_FUSED_M)
def test_mlp_bwd_fused(lib, M):
    """k_mlp_bwd_s + k_lnbwd_sum4_fin without a column sink, three times on the same scratch with a rescaled upstream gradient (anything stale from the launch before would
    be off by a factor), `partial` sized exactly as kasf.h says with a NaN guard behind it."""
    bf = torch.bfloat16
    i = R.stored(R.mlp_inputs(M, 64), "bf16", f16=("W2",))
    x, pf = _rows_in(i["x"], bf), _mlp_params_dev(i, bf, True)
    pb = _mlp_params_dev(R.stored(R.mlp_inputs(M, 64), "bf16"), bf, False)
    out, xn = _rows_out(M, 128, bf), _rows_out(M, 128, bf)
    _ok(lib.kasf_op_mlp_fwd(1, ptr(x), ptr(pf["gm"]), ptr(pf["bt"]), ptr(pf["W1"]), ptr(pf["b1"]), ptr(pf["W2"]), ptr(pf["b2"]), ptr(pf["ls"]), ptr(out), M, ptr(xn), stream()), lib)
    _tail_kept(xn, M, f"mlp_bwd_fused M={M} xn_out")
    xn[M:] = float("nan")                                  # LN(x) as the forward left it is an operand of the backward
    ranges = len(R.wg_ranges(M, 32, 64))
    part = _new(ranges * 65536 + 1024, fill=float("nan"))
    dap = _new(4 * M * 128 + 4096, bf, float("nan"))
    one = lambda *s: _new(tuple(s), fill=1.0)
    acc = dict(dW1=one(512, 128), dW2u=one(128, 512), db1=one(512), gsum=one(128), dgamma=one(128), dbeta=one(128))
    runs = []
    for scale in (0.25, -0.5, 1.0, 1.0):                   # (0.25, -0.5: exact in bf16)
        for t in acc.values():
            t.fill_(1.0)
        gin = _rows_out(M, 128, bf)
        g = _rows_in(i["gout"] * scale, bf)
        _ok(lib.kasf_op_mlp_bwd_fused(ptr(x), ptr(xn), ptr(g), ptr(pb["gm"]), ptr(pb["W1"]), ptr(pb["b1"]), ptr(pb["W2ts"]), ptr(pb["W1t"]), ptr(dap), ptr(part), ptr(acc["dW1"]),
                                      ptr(acc["dW2u"]), ptr(acc["db1"]), ptr(acc["gsum"]), ptr(gin), ptr(acc["dgamma"]), ptr(acc["dbeta"]), M, stream()), lib)
        _tail_kept(gin, M, f"mlp_bwd_fused M={M} g_in")
        _all_nan(part[ranges * 65536:], "mlp_bwd_fused partial")
        _all_nan(dap[4 * M * 128:], "mlp_bwd_fused dapart")
        runs.append(dict(g_in=gin.clone(), **{n: t.clone() for n, t in acc.items()}))
    _same_bits({n: runs[2][n] for n in ("g_in", "dW1", "dW2u")}, runs[3], f"mlp_bwd_fused M={M}")          # the fixed-order outputs (the column sums are atomics here)
    ib = R.stored(R.mlp_inputs(M, 64), "bf16")
    ref = R.mlp_bwd_ref(*_f64(ib, ("x", "gout", "gm", "bt", "W1", "b1", "W2s")), R.Exact, _back(xn[:M]), 64)
    log = Log(f"mlp_bwd_fused M={M} ranges={ranges}", "bf16", "mlp_fused")
    got = runs[3]
    log.rows("g_in", _back(got["g_in"][:M]), ref["g_in"])
    blocks = min((M + 31) // 32, 512)                      # k_lnbwd_sum4_fin's streaming workgroups: one atomicAdd each into dgamma / dbeta / gsum
    for n, adds in (("dgamma", blocks), ("dbeta", blocks), ("gsum", blocks), ("db1", ranges), ("dW1", 1), ("dW2u", 1)):
        log.red(n, _back(got[n]) - 1, ref[n], adds, no16=n == "gsum")
    log.done()


# ================================================================================================ cast
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("n", R.CAST_N)
def test_cast(lib, cd, n):
    code, dt = DT[cd]
    x = R.cast_inputs(n)
    src = _dev(torch.cat([x, torch.full((PAD,), float("nan"))]))
    dst = _new(n + PAD, dt)
    _ok(lib.kasf_op_cast(code, ptr(src), ptr(dst), n, 0, stream()), lib)
    want = x.to(dt)                                        # torch: round to nearest even; NaN stays NaN, the largest fp32 becomes inf in bf16
    got = dst[:n].cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN positions"
    bits = (lambda t: t.view(torch.int16)) if cd == "bf16" else (lambda t: t.view(torch.int32))
    assert torch.equal(bits(got)[~nan], bits(want)[~nan]), f"cast from fp32 ({cd}, n={n}) is not torch's round-to-nearest-even bit for bit"
    assert bool((dst[n:] == SENTINEL).all())
    # and back: exact
    src2 = _dev(torch.cat([want, torch.full((PAD,), float("nan"), dtype=dt)]), dt)
    back = _new(n + PAD)
    _ok(lib.kasf_op_cast(code, ptr(src2), ptr(back), n, 1, stream()), lib)
    got = back[:n].cpu()
    assert torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], want.float().view(torch.int32)[~nan]), f"cast to fp32 ({cd}, n={n})"
    assert bool((back[n:] == SENTINEL).all())


# ================================================================================================ M = 0
@pytest.mark.parametrize("cd", CDS)
def test_no_tokens(lib, cd):
    """M = 0: every entry returns 0 without a launch (kasf_launch_wgrad used to divide by a slice length of 0, kasf_launch_mlp_bwd_q by a range count of 0; the fp32
    kasf_launch_linear / _linear_res launched an empty grid, which HIP refuses) and every buffer keeps its sentinel"""
    code, dt = DT[cd]
    w = [_new((512, 512), dt) for _ in range(4)]            # stand-ins for every model-dtype operand and output
    f = [_new(512 * 512) for _ in range(8)]                 # and for every fp32 one
    S = stream()
    p = lambda k: ptr(w[k])
    q = lambda k: ptr(f[k])
    for N in (128, 512):
        assert lib.kasf_op_linear(code, p(0), p(1), q(0), p(2), 0, N, q(1), q(2), p(3), 0, S) == 0
        assert lib.kasf_op_linear(code, p(0), p(1), q(0), p(2), 0, N, None, None, None, 1, S) == 0
    assert lib.kasf_op_linear_res(code, p(0), p(1), q(0), q(1), p(2), p(3), 0, S) == 0
    for Kd in (128, 256, 384, 512):
        assert lib.kasf_op_dgrad_lnbwd(code, p(0), Kd, p(1), None, p(2), q(0), p(2), p(3), 0, q(1), q(2), 0, None, None, S) == 0
    for N, K in R.WGRAD_NK:
        assert lib.kasf_op_wgrad(code, p(0), N, p(1), K, None, None, q(0), q(1), 0, None, 0, S) == 0
        assert lib.kasf_op_wgrad(code, p(0), N, p(1), K, None, None, q(0), q(1), 0, q(2), 512 * 512, S) == 0
    assert lib.kasf_op_wgrad(code, p(0), 128, p(1), 128, q(2), q(3), q(0), q(1), 0, None, 0, S) == 0
    assert lib.kasf_op_mlp_fwd(code, p(0), q(0), q(1), p(1), q(2), p(2), q(3), q(4), p(3), 0, None, S) == 0
    assert lib.kasf_op_mlp_bwd(code, p(0), p(1), q(0), q(1), p(2), q(2), p(2), p(2), p(3), p(3), p(3), q(3), q(4), 0, S) == 0
    assert lib.kasf_op_cast(code, q(0), p(3), 0, 0, S) == 0 and lib.kasf_op_cast(code, p(0), q(0), 0, 1, S) == 0
    if cd == "bf16":
        assert lib.kasf_op_mlp_fwd(code, p(0), q(0), q(1), p(1), q(2), p(2), q(3), q(4), p(3), 0, p(3), S) == 0
        assert lib.kasf_op_mlp_bwd_fused(p(0), p(1), p(2), q(0), p(1), q(1), p(2), p(2), p(3), q(2), q(3), q(4), q(5), q(6), p(3), q(7), q(7), 0, S) == 0
        assert lib.kasf_op_dgrad_wg(p(0), 128, p(1), None, p(2), q(0), q(1), p(2), p(3), 0, q(2), q(3), q(4), None, None, None, None, None, None, None, None, 0, p(3),
                                    256 * 128 * 128 * 2, None, 0, q(5), 512 * 512, S) == 0
    torch.cuda.synchronize()
    for t in w + f:
        assert bool((t == SENTINEL).all())
