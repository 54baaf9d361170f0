"""The MLP, data-gradient and GCN backward kernels in the form a backward stage runs them: with a column sink (csrc/k_reduce.hip: one row of per-channel sums per
workgroup, added in a fixed order by k_col_finish), through kasf_op_mlp_bwd_fused_fc2, kasf_op_mlp_bwd_rows, kasf_op_dgrad_lnbwd_rows and kasf_op_gcn_bwd_rows
(include/kasf.h).  tests/test_gpu_dense.py and tests/test_gpu_gcn.py run the same kernels through their fp32-atomics branch, which the engine never takes.

The conventions are those of tests/test_gpu_dense.py (operands rounded to the storage dtype, planted rows, 64 rows of NaN behind row M, a sentinel tail on token-major
outputs, accumulators that start at 1) and its bars (dense_ref.BAR32 / DIST16, `Log`), with `adds = 1` for every per-channel sum: one addition into the accumulator
on the fixed-order path.  The GCN entry keeps the bars of tests/test_gpu_gcn.py.  On top of the comparison with the fp64 reference, every case checks
  * the scratch: sized exactly by kasf_op_sink_scratch_floats (== dense_ref's restatement), NaN at the start, 64 floats of NaN guard behind it that stay NaN;
  * stale rows: launches with the upstream gradient scaled by 0.25, -0.5 and 1 run on the SAME scratch, so a row that is added without having been written in this
    launch, or a sum that is added where it is assigned, is off by a factor;
  * two runs from identical inputs give the same bits in EVERY output, per-channel sums included;
  * token-major outputs equal the entry without scratch bit for bit, and so do the per-channel sums where one workgroup owns every row;
  * one float less of scratch: the _rows entries return 6, leave the whole scratch alone and still meet the atomics bars; the fc2 form returns 2 and writes nothing.

Kernels by test: test_mlp_bwd_fused_fc2 k_mlp_bwd_s (db1_rows) + k_lnbwd_sum4_fin<2> (part != nullptr; mlp_wfinish_body's fin branch) + k_col_finish modes 0 and 1;
test_mlp_bwd_rows k_mlp_bwd<float / bf16>; test_dgrad_lnbwd_rows k_dgrad_r<3 / 1 / 2 / 2> (non-WG) and k_dgrad_lnbwd<float / bf16> (Kd 512, and Kd 128 with add and
accumulate); test_gcn_bwd_rows k_gcn_bwd1<float / bf16>.
"""
import pytest
import torch

from tests import dense_ref as R
from tests import test_gpu_dense as D
from tests import test_gpu_gcn as G
from tests.gpu_util import DT, ptr, rel_err, stream

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
SCALES = (0.25, -0.5, 1.0, 1.0)       # (0.25 and -0.5 are exact in bf16; the last two runs are the "identical inputs" pair)
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    from kasportsformer_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _keepalive():
    """Device tensors handed to the (asynchronous) launches must outlive them (the helpers of the two modules keep them in their own lists)."""
    D._KEEP.clear()
    G._KEEP.clear()
    yield
    torch.cuda.synchronize()
    D._KEEP.clear()
    G._KEEP.clear()


def _scratch(lib, op, code, M, Kd, form, want, guard=GUARD):
    """NaN scratch of exactly the queried size with the guard behind it -> (buffer, floats); the query must equal the restatement `want`"""
    need = int(lib.kasf_op_sink_scratch_floats(op, code, M, Kd, form))
    assert need == want, f"kasf_op_sink_scratch_floats says {need}, the launcher's arithmetic restated {want}"
    return D._new(need + guard, fill=NAN), need


def _clone(d):
    return {n: t.clone() for n, t in d.items()}


def _equal_bits(a, b, names, what):
    for n in names:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs"


# ================================================================================================ bf16 MLP backward with fc2 finished
def _fc2_setup(lib, M):
    """operands on the device, LN(x) as the forward left it, the scratch buffers of the fused backward"""
    from kasportsformer_amd import _lib
    bf = torch.bfloat16
    i = R.mlp_fc2_inputs(M)
    x = D._rows_in(i["x"], bf)
    pf = D._mlp_params_dev(R.stored(R.mlp_inputs(M, 64), "bf16", f16=("W2",)), bf, True)
    pb = D._mlp_params_dev(i, bf, False)
    pb["W2"] = D._dev(i["W2"])                                # the fp32 master
    out, xn = D._rows_out(M, 128, bf), D._rows_out(M, 128, bf)
    D._ok(lib.kasf_op_mlp_fwd(1, ptr(x), ptr(pf["gm"]), ptr(pf["bt"]), ptr(pf["W1"]), ptr(pf["b1"]), ptr(pf["W2"]), ptr(pf["b2"]), ptr(pf["ls"]), ptr(out), M, ptr(xn), stream()), lib)
    D._tail_kept(xn, M, f"fc2 M={M} xn_out")
    xn[M:] = NAN
    ranges = len(R.wg_ranges(M, 32, 64))
    part = D._new(ranges * 65536 + 1024, fill=NAN)
    dap = D._new(4 * M * 128 + 4096, bf, NAN)
    scratch, need = _scratch(lib, _lib.SINK_MLP_BWD_FUSED_FC2, 1, M, 0, 0, R.fc2_scratch_floats(M))
    one = lambda *s: D._new(tuple(s), fill=1.0)
    acc = dict(dW1=one(512, 128), dW2=one(128, 512), db1=one(512), db2=one(128), dgamma=one(128), dbeta=one(128), dls2=one(128))
    return dict(i=i, x=x, xn=xn, pb=pb, ranges=ranges, part=part, dap=dap, scratch=scratch, need=need, acc=acc, M=M)


def _fc2_call(lib, s, g, gin, scratch, floats):
    pb, a = s["pb"], s["acc"]
    return lib.kasf_op_mlp_bwd_fused_fc2(ptr(s["x"]), ptr(s["xn"]), ptr(g), ptr(pb["gm"]), ptr(pb["W1"]), ptr(pb["b1"]), ptr(pb["W2ts"]), ptr(pb["W1t"]), ptr(s["dap"]),
                                         ptr(s["part"]), ptr(a["dW1"]), ptr(a["dW2"]), ptr(a["db1"]), ptr(a["db2"]), ptr(gin), ptr(a["dgamma"]), ptr(a["dbeta"]), s["M"],
                                         ptr(pb["W2"]), ptr(pb["b2"]), ptr(pb["ls"]), ptr(a["dls2"]), ptr(scratch), floats, stream())


def _fc2_reset(acc):
    for n, t in acc.items():
        t.fill_(NAN if n == "db2" else 1.0)                   # db2 = ls2 . colsum(g) is ASSIGNED: whatever the slot held must not matter


@pytest.mark.parametrize("M", R.MLP_FC2_M)
def test_mlp_bwd_fused_fc2(lib, M):
    """k_mlp_bwd_s + k_lnbwd_sum4_fin + k_col_finish exactly as block_backward runs them in bf16 mode: W2, b2, ls2, dls2 and a sink given"""
    bf = torch.bfloat16
    s = _fc2_setup(lib, M)
    i, acc, tag = s["i"], s["acc"], f"mlp_bwd_fused_fc2 M={M}"
    runs = []
    for scale in SCALES:
        _fc2_reset(acc)
        gin = D._rows_out(M, 128, bf)
        D._ok(_fc2_call(lib, s, D._rows_in(i["gout"] * scale, bf), gin, s["scratch"], s["need"]), lib)
        D._tail_kept(gin, M, tag + " g_in")
        D._all_nan(s["scratch"][s["need"]:], tag + " scratch")
        D._all_nan(s["part"][s["ranges"] * 65536:], tag + " partial")
        D._all_nan(s["dap"][4 * M * 128:], tag + " dapart")
        runs.append(dict(g_in=gin.clone(), **_clone(acc)))
    assert not bool(torch.isnan(s["scratch"][:s["need"]]).any()), tag + ": a row of the scratch was never stored"      # (512- and 384-float rows: no rounding gap)
    D._same_bits(runs[2], runs[3], tag)                       # every output, per-channel sums included
    # the entry without a sink on the same operands: g_in and dW1 (fixed order there too) bit for bit; the per-channel sums where one workgroup owns every row
    old = dict(dW1=acc["dW1"].clone().fill_(1.0), dW2u=D._new((128, 512), fill=1.0), db1=D._new(512, fill=1.0), gsum=D._new(128, fill=1.0), dgamma=D._new(128, fill=1.0),
               dbeta=D._new(128, fill=1.0), g_in=D._rows_out(M, 128, bf))
    pb = s["pb"]
    D._ok(lib.kasf_op_mlp_bwd_fused(ptr(s["x"]), ptr(s["xn"]), ptr(D._rows_in(i["gout"], bf)), ptr(pb["gm"]), ptr(pb["W1"]), ptr(pb["b1"]), ptr(pb["W2ts"]), ptr(pb["W1t"]),
                                    ptr(s["dap"]), ptr(s["part"]), ptr(old["dW1"]), ptr(old["dW2u"]), ptr(old["db1"]), ptr(old["gsum"]), ptr(old["g_in"]), ptr(old["dgamma"]),
                                    ptr(old["dbeta"]), M, stream()), lib)
    got = runs[3]
    _equal_bits(got, old, ("g_in", "dW1"), tag + " against kasf_op_mlp_bwd_fused")
    if M <= 32:                                               # one token range and one streaming workgroup
        _equal_bits(got, old, ("db1", "dgamma", "dbeta"), tag + " against kasf_op_mlp_bwd_fused (one workgroup)")
    ref = R.mlp_fc2_ref(*D._f64(i, ("x", "gout", "gm", "bt", "W1", "b1", "W2s", "W2", "b2", "ls")), R.Exact, D._back(s["xn"][:M]))
    log = D.Log(f"{tag} ranges={s['ranges']}", "bf16", "mlp_fc2")
    log.rows("g_in", D._back(got["g_in"][:M]), ref["g_in"])
    for n in ("dgamma", "dbeta", "db1", "dW1", "dW2"):
        log.red(n, D._back(got[n]) - 1, ref[n], 1)
    log.red("dls2", D._back(got["dls2"]) - 1, ref["dls2"], 2)      # two additions into the accumulator: the W2 . G term by its fin block, the b2 . colsum(g) term by k_col_finish
    log.red("db2", D._back(got["db2"]), ref["db2"], 0, no16=True)   # assigned; a plain column sum of an operand times ls2
    log.done()


@pytest.mark.parametrize("M", (33, 2049))
def test_mlp_bwd_fused_fc2_refuses_missing_scratch(lib, M):
    """this form has no atomics fallback: one float less, or no scratch at all, is error 2 before any launch, and nothing is written"""
    bf = torch.bfloat16
    s = _fc2_setup(lib, M)
    _fc2_reset(s["acc"])
    gin, g = D._rows_out(M, 128, bf), D._rows_in(s["i"]["gout"], bf)
    assert _fc2_call(lib, s, g, gin, s["scratch"], s["need"] - 1) == 2 and b"no atomics fallback" in lib.kasf_last_error()
    assert _fc2_call(lib, s, g, gin, None, 0) == 2 and _fc2_call(lib, s, g, gin, None, s["need"]) == 2
    torch.cuda.synchronize()
    assert bool((gin == D.SENTINEL).all()) and all(bool(torch.isnan(t).all()) for t in (s["scratch"], s["part"], s["dap"], s["acc"]["db2"]))
    assert all(bool((t == 1).all()) for n, t in s["acc"].items() if n != "db2")
    D._ok(_fc2_call(lib, s, g, gin, s["scratch"], s["need"]), lib)
    assert not bool(torch.isnan(s["acc"]["db2"]).any()) and not bool((s["acc"]["dls2"] == 1).all())


# ================================================================================================ generic MLP backward
@pytest.mark.parametrize("cd", D.CDS)
@pytest.mark.parametrize("M", R.MLP_BWD_M)
def test_mlp_bwd_rows(lib, cd, M):
    from kasportsformer_amd import _lib
    code, dt = DT[cd]
    i, ref = D._mlp_bwd_case(cd, M)
    x, p = D._rows_in(i["x"], dt), D._mlp_params_dev(i, dt, False)
    rows = R.mlp_bwd_rows(cd, M)
    scratch, need = _scratch(lib, _lib.SINK_MLP_BWD_ROWS, code, M, 0, 0, R.sink_floats((rows, 256)))
    tag = f"mlp_bwd_rows {cd} M={M} rows={rows}"

    def run(scale, buf, floats, want_rc=0):
        H, dZ, gin = D._rows_out(M, 512, dt), D._rows_out(M, 512, dt), D._rows_out(M, 128, dt)
        dg, db = D._new(128, fill=1.0), D._new(128, fill=1.0)
        g = D._rows_in(i["gout"] * scale, dt)
        if floats is None:
            rc = lib.kasf_op_mlp_bwd(code, ptr(x), ptr(g), ptr(p["gm"]), ptr(p["bt"]), ptr(p["W1"]), ptr(p["b1"]), ptr(p["W2ts"]), ptr(p["W1t"]), ptr(H), ptr(dZ), ptr(gin),
                                     ptr(dg), ptr(db), M, stream())
        else:
            rc = lib.kasf_op_mlp_bwd_rows(code, ptr(x), ptr(g), ptr(p["gm"]), ptr(p["bt"]), ptr(p["W1"]), ptr(p["b1"]), ptr(p["W2ts"]), ptr(p["W1t"]), ptr(H), ptr(dZ),
                                          ptr(gin), ptr(dg), ptr(db), M, ptr(buf), floats, stream())
        assert rc == want_rc, (rc, lib.kasf_last_error())
        torch.cuda.synchronize()
        for n, t in (("H", H), ("dZ", dZ), ("g_in", gin)):
            D._tail_kept(t, M, f"{tag} {n}")
        return dict(H=H, dZ=dZ, g_in=gin, dgamma=dg, dbeta=db)

    runs = []
    for scale in SCALES:
        runs.append(run(scale, scratch, need))
        D._all_nan(scratch[need:], tag + " scratch")
    D._same_bits(runs[2], runs[3], tag)
    got, old = runs[3], run(1.0, None, None)
    _equal_bits(got, old, ("H", "dZ", "g_in"), tag + " against kasf_op_mlp_bwd")
    if rows == 1:
        _equal_bits(got, old, ("dgamma", "dbeta"), tag + " against kasf_op_mlp_bwd (one workgroup)")
    short_buf = D._new(need + GUARD, fill=NAN)
    short = run(1.0, short_buf, need - 1, want_rc=6)          # falls back to the atomics, and says so
    D._all_nan(short_buf, tag + " scratch (too small: the launch must leave it alone)")
    _equal_bits(short, old, ("H", "dZ", "g_in"), tag + " short scratch against kasf_op_mlp_bwd")
    log = D.Log(tag, cd, "mlp_bwd")
    for n in ("H", "dZ", "g_in"):
        log.rows(n, D._back(got[n][:M]), ref[n])
    for n in ("dgamma", "dbeta"):
        log.red(n, D._back(got[n]) - 1, ref[n], 1)
        log.red(n + "[short]", D._back(short[n]) - 1, ref[n], rows)
    log.done()


# ================================================================================================ data gradient + LayerNorm backward
@pytest.mark.parametrize("cd", D.CDS)
@pytest.mark.parametrize("Kd,use_add,use_resid,acc,want_xn", R.DGRAD_CASES, ids=[f"Kd{c[0]}-add{int(c[1])}-resid{int(c[2])}-acc{int(c[3])}-xn{int(c[4])}" for c in R.DGRAD_CASES])
@pytest.mark.parametrize("M", R.DGRAD_M)
def test_dgrad_lnbwd_rows(lib, cd, Kd, use_add, use_resid, acc, want_xn, M):
    from kasportsformer_amd import _lib
    code, dt = DT[cd]
    i, ref = D._dgrad_case(cd, Kd, use_add, use_resid, acc, M)
    case = (Kd, use_add, use_resid, acc, want_xn)
    rows = R.dgrad_rows(cd, case, M)
    assert rows == D._adds_dgrad(cd, *case, M)
    form = _lib.SINK_FORM_RESID * use_resid + _lib.SINK_FORM_DXN_ADD * use_add + _lib.SINK_FORM_ACCUMULATE * acc + _lib.SINK_FORM_XN_OUT * want_xn
    # (the guard holds the rows of a full persistent grid: a launch that registers a row it did not take then adds NaN from the guard, not memory behind the buffer)
    scratch, need = _scratch(lib, _lib.SINK_DGRAD_LNBWD_ROWS, code, M, Kd, form, R.sink_floats((rows, 256)), max(GUARD, 256 * 256 - rows * 256 + GUARD))
    tag = f"dgrad_lnbwd_rows {cd} Kd={Kd} add={use_add} resid={use_resid} acc={acc} xn={want_xn} M={M} rows={rows}"
    base = D._dgrad_operands(i, dt, use_add, use_resid)

    def run(scale, buf, floats, want_rc=0):
        d = base if scale == 1.0 else dict(base, dy=D._rows_in(i["dy"] * scale, dt), add=D._rows_in(i["add"] * scale, dt) if use_add else None)
        if floats is None:
            return D._run_dgrad(lib, cd, i, d, Kd, acc, want_xn, M)
        out, xn = D._rows_out(M, 128, dt, i["prev"] if acc else None), D._rows_out(M, 128, dt)
        dg, db = D._new(128, fill=1.0), D._new(128, fill=1.0)
        rc = lib.kasf_op_dgrad_lnbwd_rows(code, ptr(d["dy"]), Kd, ptr(d["wt"]), ptr(d["add"]), ptr(d["x"]), ptr(d["g"]), ptr(d["resid"]), ptr(out), int(acc), ptr(dg),
                                          ptr(db), M, ptr(xn) if want_xn else None, ptr(d["b"]) if want_xn else None, ptr(buf), floats, stream())
        assert rc == want_rc, (rc, lib.kasf_last_error())
        torch.cuda.synchronize()
        D._tail_kept(out, M, tag + " out")
        D._tail_kept(xn, M, tag + " xn_out")
        return dict(out=out, xn=xn, dgamma=dg, dbeta=db)

    runs = []
    for scale in SCALES:
        runs.append(run(scale, scratch, need))
        D._all_nan(scratch[need:], tag + " scratch")
    D._same_bits(runs[2], runs[3], tag)
    got, old = runs[3], run(1.0, None, None)
    _equal_bits(got, old, ("out", "xn"), tag + " against kasf_op_dgrad_lnbwd")
    if rows == 1:
        _equal_bits(got, old, ("dgamma", "dbeta"), tag + " against kasf_op_dgrad_lnbwd (one workgroup)")
    short_buf = D._new(need + GUARD, fill=NAN)
    short = run(1.0, short_buf, need - 1, want_rc=6)
    D._all_nan(short_buf, tag + " scratch (too small: the launch must leave it alone)")
    _equal_bits(short, old, ("out", "xn"), tag + " short scratch against kasf_op_dgrad_lnbwd")
    log = D.Log(tag, cd, "dgrad")
    log.rows("out", D._back(got["out"][:M]), ref["out"])
    for n in ("dgamma", "dbeta"):
        log.red(n, D._back(got[n]) - 1, ref[n], 1)
        log.red(n + "[short]", D._back(short[n]) - 1, ref[n], rows)
    if want_xn:
        log.rows("xn_out", D._back(got["xn"][:M]), ref["xn"], no16=True)
        D._exact_rows(got["xn"][:M], i["where"], i["b"], cd, tag)
    else:
        assert bool((got["xn"] == D.SENTINEL).all())
    log.done()


# ================================================================================================ GCN backward
class _RowsRun(G.Run):
    """G.Run whose backward goes through kasf_op_gcn_bwd_rows on a given scratch"""

    def backward_rows(self, g_dev, buf, floats, want_rc=0):
        from kasportsformer_amd import _lib
        code, dt = DT[self.cd]
        f32 = torch.float32
        r, duv = G._new((self.M, G.CH), dt), G._new((self.M, 2 * G.CH), dt)
        dls1, dw, db = G._new((G.CH,), f32, 1.0), G._new((256,), f32, 1.0), G._new((256,), f32, 1.0)
        bstats = G._new((_lib.GCN_STAT_WORDS,), torch.int64, fill=-1)
        rc = self.lib.kasf_op_gcn_bwd_rows(code, ptr(g_dev), ptr(self.d["xn"]), ptr(self.y), ptr(self.coef), ptr(self.mask), ptr(self.d["ls1"]), ptr(r), ptr(duv), ptr(dls1),
                                           ptr(dw), ptr(db), ptr(bstats), self.B, self.T, self.mode, int(self.training), ptr(buf), floats, stream())
        assert rc == want_rc, (rc, self.lib.kasf_last_error())
        torch.cuda.synchronize()
        assert bool((dw[self.nodes:] == 1).all()) and bool((db[self.nodes:] == 1).all()), "d_bn_w / d_bn_b written past the node count"
        return dict(r=r, duv=duv, dls1=dls1, d_bn_w=dw, d_bn_b=db)

    def values(self, t):
        return dict(r=G._back(t["r"]), duv=G._back(t["duv"]), dls1=G._back(t["dls1"]) - 1, d_bn_w=G._back(t["d_bn_w"][:self.nodes]) - 1,
                    d_bn_b=G._back(t["d_bn_b"][:self.nodes]) - 1)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("mode,T,B", G.PARITY_CASES)
def test_gcn_bwd_rows(lib, cd, mode, T, B):
    """k_gcn_bwd1 with its dls1 rows in the sink (what block_backward passes), at the shapes and bars of test_gpu_gcn.py's backward test: fp32 1e-4, bf16
    max(3e-2, 2 x the reference's own sensitivity to the kernels' bf16 storage points); dls1 starts at 1 and takes one addition"""
    from kasportsformer_amd import _lib
    code, dt = DT[cd]
    inp = G._inputs(mode, T, B, 4)
    run = _RowsRun(lib, cd, inp, mode, T, B, 4, 1)
    ref = G.Ref(run.op, mode, T, B, 4, 1, y_stored=G._back(run.y))
    g_dev, g, frac = G._safe_g(inp["g"], ref, cd, 1e-3)
    M = run.M
    rows = R.gcn_bwd_rows(M)
    scratch, need = _scratch(lib, _lib.SINK_GCN_BWD_ROWS, code, M, 0, 0, R.sink_floats((rows, 128)))
    tag = f"gcn_bwd_rows {cd} mode={mode} T={T} B={B} rows={rows}"
    runs = []
    for scale in SCALES:
        gs = g_dev if scale == 1.0 else G._dev(g_dev.float() * scale, dt)
        runs.append(run.backward_rows(gs, scratch, need))
        D._all_nan(scratch[need:], tag + " scratch")
    D._same_bits(runs[2], runs[3], tag)
    got = runs[3]
    run.backward(g_dev)                                       # the entry without scratch: r and duv bit for bit (the BatchNorm sums are exact integer accumulators in both)
    old = dict(r=run.r, duv=run.duv, d_bn_w=run.d_bn_w, d_bn_b=run.d_bn_b)
    _equal_bits(got, old, ("r", "duv", "d_bn_w", "d_bn_b"), tag + " against kasf_op_gcn_bwd")
    short_buf = G._new((need + GUARD,), torch.float32, NAN)
    short = run.backward_rows(g_dev, short_buf, need - 1, want_rc=6)
    D._all_nan(short_buf, tag + " scratch (too small: the launch must leave it alone)")
    _equal_bits(short, old, ("r", "duv"), tag + " short scratch against kasf_op_gcn_bwd")
    want = ref.backward(g)
    hand = ref.backward_by_hand(g)
    bars = {n: G.TOL[cd] for n in want}
    if cd == "bf16":
        emu = ref.backward_by_hand(g, G._round_bf16)
        bars = {n: max(G.TOL[cd], 2 * rel_err(emu[n], hand[n])) for n in want}
    log, ok = [], True
    vals, vshort = run.values(got), run.values(short)
    for n in ("r", "duv", "dls1", "d_bn_w", "d_bn_b"):
        ok &= G._check(n, vals[n], want[n], bars[n], log)
    ok &= G._check("dls1[short]", vshort["dls1"], want["dls1"], bars["dls1"], log)
    print(f"\n[{tag}] gate-zeroed {frac:.1e}: " + "; ".join(log))
    assert ok, "; ".join(log)


# ================================================================================================ M = 0
@pytest.mark.parametrize("cd", D.CDS)
def test_no_tokens(lib, cd):
    """M = 0: the entries return 0 without a launch, with and without scratch, and every buffer keeps its sentinel (the GCN entry has no such call: batch < 1 is
    error 2 there, as in kasf_op_gcn_bwd)"""
    code, dt = DT[cd]
    w = [D._new((512, 512), dt) for _ in range(4)]
    f = [D._new(512 * 512) for _ in range(8)]
    S = stream()
    p = lambda k: ptr(w[k])
    q = lambda k: ptr(f[k])
    for sc, n in ((q(7), 512 * 512), (None, 0)):
        assert lib.kasf_op_mlp_bwd_rows(code, p(0), p(1), q(0), q(1), p(2), q(2), p(2), p(2), p(3), p(3), p(3), q(3), q(4), 0, sc, n, S) == 0
        for Kd in (128, 256, 384, 512):
            assert lib.kasf_op_dgrad_lnbwd_rows(code, p(0), Kd, p(1), None, p(2), q(0), p(2), p(3), 0, q(1), q(2), 0, None, None, sc, n, S) == 0
    assert lib.kasf_op_gcn_bwd_rows(code, p(0), p(1), p(2), q(0), q(1), q(2), p(3), p(3), q(3), q(4), q(5), q(6), 0, 27, 0, 1, q(7), 512 * 512, S) == 2
    if cd == "bf16":
        assert lib.kasf_op_mlp_bwd_fused_fc2(p(0), p(1), p(2), q(0), p(1), q(1), p(2), p(2), p(3), q(2), q(3), q(4), q(5), q(6), p(3), q(7), q(7), 0, q(0), q(1), q(2), q(3),
                                             q(7), 512 * 512, S) == 0
    torch.cuda.synchronize()
    for t in w + f:
        assert bool((t == D.SENTINEL).all())
