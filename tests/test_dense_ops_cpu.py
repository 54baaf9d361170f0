"""CPU-side checks of the linear / data-gradient / weight-gradient / MLP operator entries (include/kasf.h, kasf_op_linear ... kasf_op_cast): the two entries
tests/test_gpu_dense.py adds, the measurements its bars are derived from (tests/dense_ref.py: BAR32, DIST16), and the hand-written backward formulas of the
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
    assert _lib.ABI_VERSION == 12 and lib.kasf_version() == 12          # additive under ABI 12


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
