"""CPU-side checks of the linear / data-gradient / weight-gradient / MLP operator entries (include/kasf.h, kasf_op_linear ... kasf_op_cast): the three entries
tests/test_gpu_dense.py adds, the launcher checks and shape tables of kasf_op_wgrad_jobs, the measurements its bars are derived from (tests/dense_ref.py: BAR32, DIST16), and the hand-written backward formulas of the
reference against fp64 autograd of the forward.  No GPU."""
import pytest
import torch

from tests import dense_ref as R


@pytest.fixture(scope="module")
def lib():
    from kasportsformer_amd import _lib
    return _lib.load()


def test_symbols_and_prototypes(lib):
    from kasportsformer_amd import _lib
    for n in ("kasf_op_linear_res", "kasf_op_dgrad_wg"):
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
        assert getattr(lib, n).argtypes == _lib.SIGNATURES[n][1]
    assert len(_lib.SIGNATURES["kasf_op_dgrad_wg"][1]) == 29
    assert "kasf_op_wgrad_jobs" in _lib.SIGNATURES and lib.kasf_op_wgrad_jobs.argtypes == _lib.SIGNATURES["kasf_op_wgrad_jobs"][1]
    assert len(_lib.SIGNATURES["kasf_op_wgrad_jobs"][1]) == 25
    assert _lib.ABI_VERSION == 12 and lib.kasf_version() == 12          # additive under ABI 12


def test_wgrad_jobs_returns_zero_without_tokens(lib):
    """M = 0 passes the checks and returns 0 before any device call (host memory stands in for the arrays)"""
    import ctypes as C
    buf = C.create_string_buffer(4096 + 64)
    p = (C.addressof(buf) + 63) // 64 * 64
    arr, none, n = (C.c_void_p * 1)(p), (C.c_void_p * 1)(), (C.c_int32 * 1)(384)
    a = lambda t: C.addressof(t)
    assert lib.kasf_op_wgrad_jobs(1, a(arr), a(arr), a(n), a(arr), a(none), -1, None, None, None, None, 0, p, 0, 0, None, None, None, None, None, None, 0, None, None, None) == 0


def test_wgrad_jobs_launcher_declines_an_incomplete_fin_job(lib):
    """kasf_launch_wgrad_jobs (kernels.h; reached here through its C++ symbol, Itanium-mangled from that declaration) returns false, before any device call, for a fin
    job whose finishing workgroups would read or write through NULL: no dbias[fin_job] (its rows `brow` and `db`), one of fin_W / fin_bias / fin_ls / fin_dls missing,
    fin_job >= njobs, or N != 128 (fin_W is [128][128]).  The entry refuses all of these earlier (tests/refusal_cases.py); the engine never makes them."""
    import ctypes as C
    # The mangled name spells the launcher's parameter types, so it stands for the argtypes below: a change of the declaration in kernels.h changes the name, and this
    # lookup fails instead of calling with stale types.  Then take the new name from `nm -D --defined-only kasportsformer_amd/libkasf_hip.so | grep
    # kasf_launch_wgrad_jobs` and bring `argtypes` and `call` below in line with the new declaration.
    name = "_Z22kasf_launch_wgrad_jobsP12ihipStream_tiPKPKvS4_PKiPKPfS9_iPKfSB_SB_S7_lS7_liPK14KasfBf16ReduceS2_SB_iS7_S7_"
    assert hasattr(lib, name), "kasf_launch_wgrad_jobs is not exported under the name of its declaration in kernels.h (changed parameters, or a hidden symbol): see above"
    fn = getattr(lib, name)
    vp = C.c_void_p
    fn.restype = C.c_bool
    fn.argtypes = [vp, C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 4 + [C.c_int64, vp, C.c_int64, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    buf = C.create_string_buffer(1 << 16)
    p = (C.addressof(buf) + 63) // 64 * 64
    two, none = (vp * 2)(p, p), (vp * 2)()
    with_db = (vp * 2)(p, None)
    a = lambda t: C.addressof(t)

    def call(njobs, Ns, dbias, fin_job, fw=p, fb=p, fl=p, fd=p):
        n = (C.c_int * 2)(*Ns)
        return fn(None, njobs, a(two), a(two), a(n), a(two), a(dbias), fin_job, fw, fb, fl, fd, 1, p, 1 << 40, 0, None, None, None, 0, None, None)

    assert call(2, (128, 384), none, 0) is False                              # the defect: brow and db of the fin job were NULL and W was not
    assert call(1, (128, 384), with_db, 1) is False and call(2, (128, 384), with_db, 2) is False
    for k in range(4):
        assert call(2, (128, 384), with_db, 0, *[None if q == k else p for q in range(4)]) is False
    assert call(2, (256, 384), with_db, 0) is False
    assert call(2, (128, 384), (vp * 2)(None, p), -1) is False                # (as before: a bias gradient on a job that is not the fin job)


def test_jobs_tables_meet_the_conditions():
    """the token counts of tests/test_gpu_dense.py::test_wgrad_jobs against the launcher's arithmetic as dense_ref.jobs_splits restates it: every mix meets one token,
    a last split of one row, a split with a register tail and one without, 1 / 2 / 7 / 8 k / 8 k + r splits (the remainder branch of the XCD order), 1 / 16 / 17 /
    32 / 33 / >= 49 tiles in the finish loop, and splits of three or more 64-row ring tiles (a two-stage ring takes a stage again)"""
    assert R.jobs_splits(1, (128,)) == (1, 128) and R.jobs_splits(31744, (128,)) == (248, 128) and R.jobs_splits(31745, (128,)) == (125, 256)
    assert R.jobs_splits(24577, (128, 384)) == (49, 512) and R.jobs_splits(7937, (128, 128, 256)) == (32, 256) and R.jobs_splits(10625, (384,)) == (42, 256)
    assert R.jobs_splits(40000, (128, 384)) == (53, 768) and R.jobs_splits(7936, (512,)) == (62, 128)
    assert R.jobs_partial_floats(129, (128, 384), 0) == 2 * 512 * 128 + 2 * 128 and R.jobs_partial_floats(129, (384,), -1) == 2 * 384 * 128
    for mix, (Ns, fin_job, reds, ext) in R.JOBS_MIXES.items():
        cases = R.jobs_cases(mix)
        Ms = [M for M, _ in cases]
        assert Ms[0] == 1 and max(Ms) <= 32000, mix
        sp = {M: R.jobs_splits(M, Ns) for M in Ms}
        last = {M: M - (s - 1) * sl for M, (s, sl) in sp.items()}            # rows of the last split
        assert any(s > 1 and last[M] == 1 for M, (s, _) in sp.items()), mix
        assert any(last[M] % 64 != 0 for M in Ms) and any(last[M] % 64 == 0 for M in Ms), mix            # a last split with a register tail, and one without
        assert any(s > 1 and last[M] > 64 and last[M] % 64 != 0 for M, (s, _) in sp.items()), mix          # ring tiles AND a tail in one split
        counts = {s for s, _ in sp.values()}
        assert {1, 2, 7, 16, 17, 32, 33} <= counts and max(counts) >= 49, (mix, counts)
        assert any(s % 8 == 0 for s in counts) and any(s > 8 and s % 8 != 0 for s in counts) and any(s < 8 for s in counts)
        assert any(sl >= 192 for _, sl in sp.values()), mix
        parts = {p for _, p in cases}
        assert parts == set(R.JOBS_PARTS[mix]), mix            # every listed number of parts is used by some case
        if ext:
            assert {1, 16, 17, 33} <= parts and max(parts) >= 49, mix
    assert {1, 17, 256} <= set(R.JOBS_PARTS["att1_red"]) and {2, 32, 49} <= set(R.JOBS_PARTS["one_red2"])
    # the isolation case's redraw changes job 1 and nothing else
    a, b = R.jobs_inputs("att2", 2049, 0), R.jobs_inputs("att2", 2049, 0, 1)
    assert torch.equal(a["G"][0], b["G"][0]) and torch.equal(a["X"][0], b["X"][0]) and torch.equal(a["W"], b["W"]) and not torch.equal(a["G"][1], b["G"][1])


def test_wgrad_jobs_reference_is_autograd_of_the_projection():
    """the fin job's and the ext job's algebra: out = ls (x W^T + bias) with upstream gradient g"""
    i = R.jobs_inputs("att2", 129, 0)
    G, X, fin_job, W, bias, ls, red, ep, eb = R.jobs_sel(i, torch.float64)
    Wl, bl, lsl = (t.clone().requires_grad_(True) for t in (W, bias, ls))
    ((lsl * (X[0] @ Wl.T + bl)) * G[0]).sum().backward()
    r = R.wgrad_jobs_ref(G, X, fin_job, W, bias, ls, red, ep, eb)
    assert R.rel_err(r["dw0"], Wl.grad) < 1e-12 and R.rel_err(r["db"], bl.grad) < 1e-12 and R.rel_err(r["dls"], lsl.grad) < 1e-12
    assert R.rel_err(r["dw1"], G[1].T @ X[1]) == 0
    i = R.jobs_inputs("ext_bone", 129, 17)
    G, X, fin_job, W, bias, ls, red, ep, eb = R.jobs_sel(i, torch.float64)
    r = R.wgrad_jobs_ref(G, X, fin_job, W, bias, ls, red, ep, eb)
    want = R.ls_algebra(ep.sum(0), eb.sum(0), W, bias, ls)
    assert all(torch.equal(r[n], w) for n, w in zip(("ext_dw", "ext_db", "dls"), want)) and set(r) == {"dw0", "dw1", "ext_dw", "ext_db", "dls"}
    assert R.jobs_no16("dls", i) and not R.jobs_no16("dls", R.jobs_inputs("att2", 129, 0)) and R.jobs_no16("red1", i) and not R.jobs_no16("dw0", i)


def test_launcher_arithmetic_restated_by_the_reference():
    """the grids the reference restates (token ranges of the bf16 partial tiles, split counts of kasf_op_wgrad) at the shapes the issue names"""
    rows = lambda M: len(R.wg_ranges(M))
    assert rows(1) == 1 and rows(8192) == 256 and rows(8193) == 129 and R.wg_ranges(8193)[-1] == (8192, 8193)
    assert rows(16417) == 172 and R.wg_ranges(16417)[0] == (0, 96) and R.wg_ranges(16417)[-1] == (16416, 16417)                  # three tiles per range: a two-slot ring reuses a slot
    assert rows(24577) == 193 and R.wg_ranges(24577)[0] == (0, 128) and R.wg_ranges(24577)[-1] == (24576, 24577)
    fused = lambda M: R.wg_ranges(M, 32, 64)
    assert len(fused(2048)) == 64 and len(fused(2049)) == 33 and fused(2049)[-1] == (2048, 2049)
    assert len(fused(10273)) == 54 and fused(10273)[0] == (0, 192)                  # six tiles per range: one more than the five-slot ring
    assert R.wgrad_splits(128, 128, 31743)[0] == 248 and R.wgrad_splits(128, 128, 31745)[0] == 125 and R.wgrad_splits(128, 128, 127)[0] == 1
    assert R.wgrad_splits(512, 128, 31745)[0] == 50 and R.wgrad_splits(128, 128, 129)[0] == 2
    assert R.second_walk_row(8192) is None and R.second_walk_row(8193) == 32 and R.second_walk_row(2049, 32, 64) == 32


def test_plants():
    g = R.gen(0)
    x, where = R.plant(torch.randn(8193, 128, generator=g), g, 32)
    assert where["const"] == [0, 32, 8192] and where["zero"] == [1, 33, 8191] and where["big"] == [4, 36, 8188]
    assert bool((x[0] == 0.75).all()) and bool((x[8192] == -3).all()) and bool((x[1] == 0).all())
    assert 0.5e-6 < float(x[2].var()) < 2e-6 < R.LN_EPS and 30 < float(x[3].mean()) < 34 and float(x[4].abs().max()) > 1e3
    x, where = R.plant(torch.randn(1, 128, generator=g), g)
    assert where["const"] == [0] and sum(len(v) for v in where.values()) == 1
    # a constant row of at most 8 significant bits: LN(x) is beta exactly in fp32, whatever the order of the sums; a tiny row is 301.5 x, not 1000 x
    gm, bt = R.ln_params(g)
    x, where = R.plant(torch.randn(40, 128, generator=g), g)
    y = R.ln(x, gm, bt)
    for r in where["const"] + where["zero"]:
        assert torch.equal(y[r], bt)
    t = where["tiny"][0]
    ratio = float(((y[t] - bt) / gm / (x[t] - x[t].mean())).mean())
    assert abs(ratio - (float(x[t].var(unbiased=False)) + 1e-5) ** -0.5) < 1e-2 and 280 < ratio < 316


def test_layernorm_backward_formula_is_autograd_of_the_forward():
    g = R.gen(11)
    x, _ = R.plant(torch.randn(40, 128, generator=g).double(), g)
    x = x.requires_grad_(True)
    gm, bt = (t.double().requires_grad_(True) for t in R.ln_params(g))
    dxn = torch.randn(40, 128, generator=g).double()
    R.ln(x, gm, bt).backward(dxn)
    dx, dgamma, dbeta = R.ln_bwd(dxn, x.detach(), gm.detach())
    assert R.row_err(dx, x.grad)[0] < 1e-9 and R.rel_err(dgamma, gm.grad) < 1e-9 and R.rel_err(dbeta, bt.grad) < 1e-9


def test_dgrad_reference_is_autograd_of_the_linear():
    i = R.to(R.dgrad_inputs(256, 65, True), torch.float64)
    x, gm, bt = i["x"].requires_grad_(True), i["g"].requires_grad_(True), i["b"].requires_grad_(True)
    W = i["wt"].T.clone().requires_grad_(True)            # [Kd,128]
    xn = R.ln(x, gm, bt)
    ((xn @ W.T) * i["dy"]).sum().backward(retain_graph=True)
    (xn * i["add"]).sum().backward()
    r = R.dgrad_wg_ref(i["dy"], i["wt"], i["add"], x.detach(), gm.detach(), i["resid"], i["prev"], bt.detach(), True, i["o"], i["pw"], i["pb"], i["pls"])
    assert R.row_err(r["out"], x.grad + i["resid"] + i["prev"])[0] < 1e-9
    assert R.rel_err(r["dgamma"], gm.grad) < 1e-9 and R.rel_err(r["dbeta"], bt.grad) < 1e-9 and R.rel_err(r["dw"], W.grad) < 1e-9
    assert R.rel_err(r["dbias"], i["dy"].sum(0)) < 1e-12
    # the PROJ form: out_proj = resid_in + ls (o Wp^T + bp) with upstream gradient `resid` (the block's g_mid)
    pw, pb, pls = (i[k].clone().requires_grad_(True) for k in ("pw", "pb", "pls"))
    ((pls * (i["o"] @ pw.T + pb)) * i["resid"]).sum().backward()
    assert R.rel_err(r["dproj_w"], pw.grad) < 1e-9 and R.rel_err(r["dproj_b"], pb.grad) < 1e-9 and R.rel_err(r["dproj_ls"], pls.grad) < 1e-9


def test_mlp_backward_formulas_are_autograd_of_the_forward():
    """dZ, the LayerNorm backward and the UNSCALED dW2 / gsum contract (dW2 = ls[:, None] dW2u, db2 = ls gsum) of mlp_bwd_ref against autograd of mlp_fwd_ref"""
    i = R.to(R.mlp_inputs(459), torch.float64)
    leaf = {k: i[k].clone().requires_grad_(True) for k in ("x", "gm", "bt", "W1", "b1", "W2", "b2")}
    f = R.mlp_fwd_ref(leaf["x"], leaf["gm"], leaf["bt"], leaf["W1"], leaf["b1"], leaf["W2"], leaf["b2"], i["ls"])
    f["z"].retain_grad()
    f["out"].backward(i["gout"])
    z = f["z"].detach()
    assert float(z.max()) > 12 and float(z.min()) < -12 and int((z[:, 7].abs() > 6).sum()) >= 2            # the planted units reach the tails on some tokens
    for fused in (None, 64):
        b = R.mlp_bwd_ref(i["x"], i["gout"], i["gm"], i["bt"], i["W1"], i["b1"], i["ls"][:, None] * i["W2"], R.Exact, None, fused)
        assert R.row_err(b["dZ"], f["z"].grad)[0] < 1e-9 and R.row_err(b["g_in"], leaf["x"].grad)[0] < 1e-9 and R.row_err(b["H"], f["H"].detach())[0] < 1e-12
        for got, want in ((b["dgamma"], leaf["gm"].grad), (b["dbeta"], leaf["bt"].grad), (b["dW1"], leaf["W1"].grad), (b["db1"], leaf["b1"].grad),
                          (i["ls"][:, None] * b["dW2u"], leaf["W2"].grad), (i["ls"] * b["gsum"], leaf["b2"].grad)):
            assert R.rel_err(got, want) < 1e-9


def test_fc2_finish_is_autograd_of_the_forward():
    """dW2 (SCALED), db2 and dls2 of mlp_fc2_ref -- dense_ref.ls_algebra on the unscaled dW2u and gsum of the fused backward -- against fp64 autograd of mlp_fwd_ref
    with respect to W2, b2 and ls"""
    i = R.to(R.mlp_inputs(459, 64), torch.float64)
    leaf = {k: i[k].clone().requires_grad_(True) for k in ("W2", "b2", "ls")}
    R.mlp_fwd_ref(i["x"], i["gm"], i["bt"], i["W1"], i["b1"], leaf["W2"], leaf["b2"], leaf["ls"])["out"].backward(i["gout"])
    r = R.mlp_fc2_ref(i["x"], i["gout"], i["gm"], i["bt"], i["W1"], i["b1"], i["ls"][:, None] * i["W2"], i["W2"], i["b2"], i["ls"])
    for got, want in ((r["dW2"], leaf["W2"].grad), (r["db2"], leaf["b2"].grad), (r["dls2"], leaf["ls"].grad)):
        assert R.rel_err(got, want) < 1e-9
    # the operands of the entry: W2 is the fp32 master, W2s the bf16 copy of ls W2
    j, raw = R.mlp_fc2_inputs(33), R.mlp_inputs(33, 64)
    assert torch.equal(j["W2"], raw["W2"]) and torch.equal(j["W2s"], (raw["ls"][:, None] * raw["W2"]).to(torch.bfloat16).float())
    assert not torch.equal(j["W2"], j["W2"].to(torch.bfloat16).float())


def test_sink_scratch_query_is_the_launchers_arithmetic(lib):
    """kasf_op_sink_scratch_floats (computed by the helpers the launchers call) against dense_ref's restatement of each launch's requests of the column sink, at the
    listed shapes and around every edge of the grids: needs no device"""
    from kasportsformer_amd import _lib
    for n, count in (("kasf_op_sink_scratch_floats", 5), ("kasf_op_mlp_bwd_rows", 18), ("kasf_op_mlp_bwd_fused_fc2", 25), ("kasf_op_dgrad_lnbwd_rows", 18),
                     ("kasf_op_gcn_bwd_rows", 20)):
        assert n in _lib.SIGNATURES and hasattr(lib, n) and getattr(lib, n).argtypes == _lib.SIGNATURES[n][1] and len(_lib.SIGNATURES[n][1]) == count, n
    q = lib.kasf_op_sink_scratch_floats
    edges = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385, 16417, 24577, 40003, 65637, 176256)
    for M in sorted(set(edges + R.MLP_FC2_M + R.MLP_BWD_M + R.DGRAD_M)):
        assert q(_lib.SINK_MLP_BWD_FUSED_FC2, 1, M, 0, 0) == R.fc2_scratch_floats(M), M
        assert q(_lib.SINK_GCN_BWD_ROWS, 0, M, 0, 0) == q(_lib.SINK_GCN_BWD_ROWS, 1, M, 0, 0) == R.sink_floats((R.gcn_bwd_rows(M), 128)), M
        for code, cd in ((0, "fp32"), (1, "bf16")):
            assert q(_lib.SINK_MLP_BWD_ROWS, code, M, 0, 0) == R.sink_floats((R.mlp_bwd_rows(cd, M), 256)), (cd, M)
            for case in R.DGRAD_CASES:
                Kd, add, resid, acc, xn = case
                form = _lib.SINK_FORM_RESID * resid + _lib.SINK_FORM_DXN_ADD * add + _lib.SINK_FORM_ACCUMULATE * acc + _lib.SINK_FORM_XN_OUT * xn
                assert q(_lib.SINK_DGRAD_LNBWD_ROWS, code, M, Kd, form) == R.sink_floats((R.dgrad_rows(cd, case, M), 256)), (cd, case, M)
    assert R.fc2_scratch_floats(1) == 512 + 384 and R.fc2_scratch_floats(16417) == 58 * 512 + 512 * 384 and R.sink_floats((1, 100), (3, 50)) == 128 + 192
    assert R.gcn_bwd_rows(68) == 5 and R.gcn_bwd_rows(8192) == 512 and R.gcn_bwd_rows(65637) == 512
    assert min((16417 + 31) // 32, 512) == 512 < (16417 + 31) // 32                  # the shape at which k_lnbwd_sum4_fin's streaming workgroups walk twice
    # the fc2 form: M = 0 returns 0 before any device call; a missing or short scratch is refused (error 2), never fallen back from
    import ctypes as C
    buf = C.create_string_buffer(4096 + 64)
    p = (C.addressof(buf) + 63) // 64 * 64
    assert lib.kasf_op_mlp_bwd_fused_fc2(*[p] * 17, 0, *[p] * 5, 16, None) == 0
    assert lib.kasf_op_mlp_bwd_fused_fc2(*[p] * 17, 33, p, p, p, p, None, 0, None) == 2
    assert lib.kasf_op_mlp_bwd_fused_fc2(*[p] * 17, 33, *[p] * 5, R.fc2_scratch_floats(33) - 1, None) == 2 and b"no atomics fallback" in lib.kasf_last_error()
    assert not any(buf.raw)


def test_sensitivities_are_within_the_bars():
    """BAR32 is 8 x what a plain fp32 evaluation of the reference loses against the fp64 one, DIST16 what the reference moves by when the 16-bit storage points of
    the bf16 kernels are rounded, each at the op's largest listed shape with the plants in.  Re-measured here: both evaluations must stay within
    the tables, no fp32 bar may exceed 1e-4 and no bf16 bar 3e-2 (what tests/test_gpu_ops.py holds today)."""
    s32, s16 = R.measure("fp32"), R.measure("bf16")
    assert set(s32) == set(R.BAR32) == set(R.DIST16) == set(s16)
    for op in R.BAR32:
        w32, w16 = max(s32[op].values()), max(s16[op].values())
        print(f"{op}: fp32 " + ", ".join(f"{k} {v:.2e}" for k, v in s32[op].items()) + f" -> 8 x {w32:.2e} = {8 * w32:.2e}, bar32 {R.BAR32[op]:.1e}")
        print(f"{op}: 16-bit points " + ", ".join(f"{k} {v:.2e}" for k, v in s16[op].items()) + f" -> {w16:.2e}, DIST16 {R.DIST16[op]:.1e}, c {R.c16(op):.1e}")
        assert 0 < w32 <= R.BAR32[op] <= 1e-4, (op, s32[op])
        assert w16 <= R.DIST16[op] and R.c16(op) <= 3e-2, (op, s16[op])
        assert (w16 == 0) == (op == "linear_res")


def test_cast_reference_values():
    x = R.cast_inputs(128)
    b = x.to(torch.bfloat16)
    assert bool(torch.isnan(b[-12])) and bool(torch.isinf(b[-11])) and float(b[-11]) > 0      # NaN stays NaN; the largest fp32 rounds to +inf in bf16
    assert float(b[-9]) == 3.3895313892515355e38 and float(b[-8]) == 1.0 and float(b[-7]) == 1.0 + 2.0 ** -6      # ties go to the even mantissa, both ways
    assert float(b[-6]) == 1.0 + 2.0 ** -7 and float(b[-5]) == 2.0
