"""CPU-side checks of the attention operator entries (include/kasf.h, kasf_op_attention_fwd ... kasf_op_attn_block_fwd): the entry tests/test_gpu_attn.py adds, the
measurements its bars are derived from (tests/attn_ref.py: BAR32, DIST16), the hand-written backward of the reference against fp64 autograd of the forward, and the
launchers' group-to-workgroup arithmetic as the reference restates it, at the shapes the tables name for it.  No GPU."""
import pytest
import torch

from tests import attn_ref as R

F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    from kasportsformer_amd import _lib
    return _lib.load()


def test_symbol_and_prototype(lib):
    from kasportsformer_amd import _lib
    assert "kasf_op_attn_block_fwd" in _lib.SIGNATURES and hasattr(lib, "kasf_op_attn_block_fwd")
    assert lib.kasf_op_attn_block_fwd.argtypes == _lib.SIGNATURES["kasf_op_attn_block_fwd"][1] and len(_lib.SIGNATURES["kasf_op_attn_block_fwd"][1]) == 21
    assert _lib.ABI_VERSION == 12 and lib.kasf_version() == 12          # additive under ABI 12


def test_an_empty_batch_returns_0_after_the_checks(lib):
    """batch = 0 reached a launch with an empty grid before (units = 0); the refusals in front of it are held by tests/test_refusals_cpu.py"""
    import ctypes as C
    buf = C.create_string_buffer(4096 + 64)
    p = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)
    for dt in (0, 1):
        assert lib.kasf_op_attention_fwd(dt, p, 384, p, p, 384, p, 0, 4, 1, None) == 0
        assert lib.kasf_op_attention_bwd(dt, p, 384, p, p, 384, p, p, 384, p, p, 384, 0, 4, 0, None) == 0
        assert lib.kasf_op_attention_fwd_heads(dt, p, 128, p, p, 256, p, 0, 4, 1, 4, None) == 0
        assert lib.kasf_op_attention_bwd_heads(dt, p, 128, p, p, 256, p, p, 128, p, p, 256, 0, 4, 1, 2, None) == 0
    assert lib.kasf_op_attn_block_fwd(0, p, None, p, p, None, None, p, None, p, p, p, None, None, None, None, C.c_void_p(p.value + 2048), 0, 4, 1, None) == 0
    assert lib.kasf_op_attention_bwd_fused_do(p, 384, p, p, 384, p, p, p, 384, p, p, 384, 0, 4, 1, 0, None, None, None) == 2      # (this one always refused it)


def test_block_bwd_symbol_and_empty_batch(lib):
    import ctypes as C
    from kasportsformer_amd import _lib
    sig = _lib.SIGNATURES["kasf_op_attn_block_bwd"][1]
    assert lib.kasf_op_attn_block_bwd.argtypes == sig and len(sig) == 40
    buf = C.create_string_buffer(8192 + 64)
    p = C.c_void_p((C.addressof(buf) + 63) // 64 * 64)
    o = C.c_void_p(p.value + 4096)
    self_form = [0, p, None, p, p, p, None, None, p, None, None, p, p, p, p, o, None, p, None, p, None, p, p, None, None, p, None, p, p, p]
    assert lib.kasf_op_attn_block_bwd(*self_form, p, 0, p, 256 * 128 * 128 * 2 + 256 * 128 * 4, p, 64, 0, 4, 1, None) == 0          # batch = 0: after the checks, no launch


def test_block_bwd_tables_meet_the_grid():
    """the shapes of tests/test_gpu_attn.py::test_block_bwd against kasf_launch_attn_block_bwd's arithmetic as attn_ref.block_bwd_grid restates it"""
    g = lambda mode, B, T: R.block_bwd_grid(B, T, mode)
    assert g(0, 1, 1) == (1, 1, 1) and g(0, 255, 1) == (255, 1, 255) and g(0, 256, 1) == (256, 1, 256)
    assert g(0, 257, 1) == (256, 2, 129)                                  # 129 active workgroups, 127 that return at once; the last owns one group
    assert g(0, 513, 1) == (256, 3, 171)                                  # a third walk
    assert g(1, 16, 17) == (256, 2, 136) and g(1, 16, 27) == (256, 2, 136) and g(1, 31, 32) == (256, 3, 176) and 31 * 17 - 175 * 3 == 2      # a short last range
    assert g(1, 1, 4) == (17, 1, 17)
    cases = [c for v in R.BLOCK_BWD.values() for c in v]
    assert len(cases) == 17 and all(R.group_len(T, m) <= 32 for m, B, T in cases)
    assert {R.group_len(T, m) for m, B, T in R.BLOCK_BWD["t9"]} == {4, 9, 16, 17} and {R.group_len(T, m) for m, B, T in R.BLOCK_BWD["t16"]} == {18, 27, 31, 32}
    assert {g(*c)[1] for c in cases} == {1, 2, 3}
    for bone in (0, 1):                                                    # groups shorter than 8 positions carry two planted rows each, the others five
        i = R.block_bwd_inputs(bone, 1, 1, 4)
        rows = sorted(r for v in i["where"].values() for r in v)
        assert R.bwd_planted_groups(1, 4, 1) == [0, 16] and rows == [0, 17, 16 + 2 * 17, 16 + 3 * 17]            # positions 0, 1 of track 0; positions 3, 2 of track 16
        assert i["where"]["const"] == [0] and i["where"]["zero"] == [17]
        i = R.block_bwd_inputs(bone, 1, 16, 17)
        assert R.bwd_planted_groups(16, 17, 1) == [0, 1, 271] and sum(len(v) for v in i["where"].values()) == 15
        assert bool((i["wq"][48:64] == 0).all()) and float(i["g_mid"].abs().max()) > 0


def test_block_bwd_reference_is_autograd_of_the_block_forward():
    """block_bwd_ref (no rounding) against fp64 autograd of block_ref's forward for the upstream gradient g_mid, both forms"""
    for bone in (0, 1):
        mode, B, T = 1, 2, 9
        i = {k: (v.double() if torch.is_tensor(v) else v) for k, v in R.block_bwd_inputs(bone, mode, B, T).items()}
        i["wts"] = (i["ls1"][:, None] * i["proj_w"]).T.contiguous()          # (the operand is this product formed in fp32: formed in fp64 here)
        leaf = {n: i[n].clone().requires_grad_(True) for n in ("x", "xl", "ln_g", "ln_b", "lnl_g", "lnl_b", "wq", "wkv", "proj_w", "proj_b", "ls1") if i[n] is not None}
        f = dict(i, **leaf, wproj=leaf["proj_w"], bproj=leaf["proj_b"])
        R.block_ref(f, B, T, mode)["x_mid"].backward(i["g_mid"])
        r = R.block_bwd_ref(i, B, T, mode)
        e = lambda got, want: float((got - want).abs().max() / want.abs().max())
        pairs = [(r["out"], leaf["x"].grad), (r["dgamma"], leaf["ln_g"].grad), (r["dbeta"], leaf["ln_b"].grad), (r["dproj_w"], leaf["proj_w"].grad),
                 (r["dproj_b"], leaf["proj_b"].grad), (r["dls1"], leaf["ls1"].grad)]
        if bone:
            pairs += [(r["out_limb"] - i["outl0"], leaf["xl"].grad), (r["dgamma_l"], leaf["lnl_g"].grad), (r["dbeta_l"], leaf["lnl_b"].grad), (r["dw_mix"], leaf["wq"].grad),
                      (r["dw_kv"], leaf["wkv"].grad)]
        else:
            pairs += [(r["dw_mix"], leaf["wq"].grad)]
        assert all(e(a, b) < 1e-9 for a, b in pairs), [e(a, b) for a, b in pairs]


@pytest.fixture(scope="module")
def measured():
    return {w: R.measure(w) for w in ("fp32", "bf16")}


def test_fp32_sensitivity_is_within_the_bars(measured):
    m = measured["fp32"]
    print("\n[attn fp32 distance] " + "; ".join(f"{k} {v:.2e} (bar {R.BAR32[k]:.0e})" for k, v in sorted(m.items())))
    assert set(m) == set(R.BAR32)
    for k, v in m.items():
        assert 8 * v <= R.BAR32[k] <= 1e-4, (k, v)
        assert R.BAR32[k] <= 32 * v, f"{k}: the bar is more than 4 x what it is derived from ({v:.2e})"


def test_bf16_distance_is_within_the_bars(measured):
    m = measured["bf16"]
    print("\n[attn bf16 distance] " + "; ".join(f"{k} {v:.2e} (DIST16 {R.DIST16[k]:.1e}, c {R.c16(k):.1e})" for k, v in sorted(m.items())))
    assert set(m) == set(R.DIST16)
    for k, v in m.items():
        assert v <= R.DIST16[k] and R.c16(k) <= 3e-2, (k, v)
        assert R.DIST16[k] <= 2 * v + 1e-12, f"{k}: DIST16 is more than 2 x what was measured ({v:.2e})"


@pytest.mark.parametrize("H,mode,B,T", [(8, 1, 1, 33), (4, 0, 2, 3), (2, 1, 1, 5), (16, 1, 1, 9)])
def test_backward_formula_is_autograd_of_the_forward(H, mode, B, T):
    for level in ("strong", "mild"):
        i = R.core_inputs(H, mode, B, T, level)
        qg, kg, vg, dog = (R.to_groups(i[n].double(), B, T, mode) for n in ("q", "k", "v", "d_o"))
        leaves = [t.clone().requires_grad_(True) for t in (qg, kg, vg)]
        f = R.core_fwd(*leaves, H)
        f["o"].backward(dog)
        b = R.core_bwd(qg, kg, vg, dog, H)
        for n, leaf in zip(("dq", "dk", "dv"), leaves):
            assert float((b[n] - leaf.grad).abs().max()) <= 1e-9 * max(1.0, float(leaf.grad.abs().max())), (n, level)
        # the kt kernels' form (P from lse, delta from o) is the same backward
        k = R.core_bwd(qg, kg, vg, dog, H, R.Exact, f["o"].detach(), f["lse"].detach())
        for n in ("dq", "dk", "dv"):
            assert float((k[n] - b[n]).abs().max()) <= 1e-9 * max(1.0, float(b[n].abs().max())), (n, level)
        # equal keys: dq is 0; zero queries: dk is 0 (the blocks the measure takes the group's scale for)
        d = 128 // H
        for n in ("dq", "dk"):
            for G, h in i["zero"][n].nonzero().tolist():
                blk = b[n][G, :, h * d:(h + 1) * d]
                assert float(blk.abs().max()) <= 1e-12 * float(b[n][G].abs().max()), (n, G, h)


def test_lse_is_consistent_with_o():
    H, mode, B, T = 8, 1, 1, 40
    i = R.core_inputs(H, mode, B, T, "strong")
    qg, kg, vg = (R.to_groups(i[n].double(), B, T, mode) for n in ("q", "k", "v"))
    f = R.core_fwd(qg, kg, vg, H)
    P = torch.exp(R._scores(qg, kg, H) - f["lse"].transpose(1, 2).unsqueeze(-1))
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    assert float((R._merge(P @ R._heads(vg, H)) - f["o"]).abs().max()) < 1e-10 * float(f["o"].abs().max())
    # the planted heads do what they are there for: scores beyond fp32's exp range, a one-hot softmax, o = mean(v) under zero queries and equal keys
    s = R._scores(qg, kg, H)
    where = R.plant_heads(H, qg.shape[0])
    assert float(s[:, where["offset"][0]].min()) > 40 and 66 < float(s[:, where["offset"][0]].mean()) < 74 and float(s[:, where["offset"][0]].max()) > 88.8
    assert float((s[:, where["peaked"][0]].amax(-1) > 88.8).double().mean()) > 0.1            # rows of the peaked head with a score past fp32's exp range
    assert float(P[:, where["peaked"][0]].amax(-1).median()) > 0.999
    for p in ("zeroq", "eqk"):
        h = where[p][0]
        assert float((f["o"][:, :, 16 * h:16 * h + 16] - vg[:, :, 16 * h:16 * h + 16].mean(1, keepdim=True)).abs().max()) < 1e-12
    assert torch.equal(R.from_groups(R.to_groups(i["q"], B, T, mode), B, T, mode), i["q"])


def test_groups_and_tokens():
    for mode, B, T in ((0, 2, 3), (1, 2, 3)):
        x = torch.arange(B * T * 17, dtype=torch.float32)[:, None].expand(-1, 2).contiguous()
        g = R.to_groups(x, B, T, mode)
        for G in range(R.n_groups(B, T, mode)):
            for p in range(R.group_len(T, mode)):
                assert int(g[G, p, 0]) == R.token_of(G, p, T, mode)
        assert torch.equal(R.from_groups(g, B, T, mode), x)


def test_launcher_arithmetic_and_the_shape_tables():
    """every "second walk", "short last range" and "empty workgroup" the tables of attn_ref.py (and the docstring of tests/test_gpu_attn.py) name is one"""
    def walk(bone, mode, B, T):
        kernel, grid = R.block_grid(bone, B, T, mode)
        per, owned, empty = R.wg_walks(R.n_groups(B, T, mode), grid)
        return kernel, grid, per, owned[-1][1] - owned[-1][0], empty

    assert walk(0, 0, 1, 1) == ("flat", 1, 1, 1, 0) and walk(0, 0, 2, 1) == ("flat", 1, 2, 2, 0)
    assert walk(0, 0, 3, 1) == ("flat", 2, 2, 1, 0)                                   # two workgroups, the last with one frame
    assert walk(0, 0, 32, 1)[:3] == ("flat", 16, 2) and 32 * 17 % 32 == 0              # 17 full tiles, a frame ends exactly on a tile border
    assert walk(0, 0, 1025, 1) == ("flat", 512, 3, 2, 170)                             # self: per 3, short last range, empty workgroups
    assert walk(1, 0, 1025, 1) == ("flat", 256, 5, 5, 51)
    assert walk(0, *R.BLOCK_LONG[0])[:3] == ("flat", 512, 49) and walk(1, *R.BLOCK_LONG[1])[:3] == ("flat", 256, 49)
    assert sorted({17 * j % 48 for j in range(49)}) == list(range(48))               # every rolling offset of the 48-row q | k | v tiles
    assert walk(0, 1, 31, 32) == ("rp", 512, 2, 1, 248) and walk(1, 1, 31, 32) == ("rp", 256, 3, 2, 80)
    assert walk(1, 1, 46, 27) == ("rp", 256, 4, 2, 60) and walk(0, 1, 46, 27)[:3] == ("rp", 512, 2)
    assert walk(0, 1, 16, 81) == ("rp3", 256, 2, 2, 120) and walk(0, 1, 31, 96) == ("rp3", 256, 3, 2, 80)
    for name, cases in R.BLOCK.items():
        for mode, B, T in cases:
            assert R.block_grid(0, B, T, mode)[0] == R.block_grid(1, B, T, mode)[0] == name
    # fused-d_o backward
    for name, cases in R.FUSED_DO.items():
        for mode, B, T in cases:
            assert R.fused_do_grid(B, T, mode, name.startswith("kt"))[0] == name, (name, mode, B, T)
    k, grid, _ = R.fused_do_grid(31, 32, 1, False)
    assert (k, grid) == ("pers16", 512) and R.wg_walks(527, grid) [0] == 2 and R.wg_walks(527, grid)[2] == 248     # a second walk, and workgroups with no group
    assert R.wg_walks(41 * 27, R.fused_do_grid(41, 27, 0, False)[1])[0] == 3
    assert [R.fused_do_grid(B, 81, 1, True)[1:] for B in (1, 3, 16)] == [(48, 24), (112, 56), (544, 272)]             # 17, 51, 272 groups: 24 and 56 slots have room to spare
    # the cores' instantiations
    assert [R.core_kernel("bf16", 8, T, 1)[0] for T in (32, 33, 96, 97, 128, 129, 192, 193, 256)] == \
        [f"k_attn_fwd_mfma<{n}>" for n in (1, 3, 3, 4, 4, 6, 6, 8, 8)]
    assert [R.core_kernel("bf16", 8, T, 1)[1] for T in (32, 33, 96, 97, 129, 193)] == \
        ["k_attn_bwd_mfma<1>", "k_attn_bwd_long<3>", "k_attn_bwd_long<3>", "k_attn_bwd_2p<4>", "k_attn_bwd_2p<6>", "k_attn_bwd_2p<8>"]
    assert R.core_kernel("bf16", 8, 257, 1) == ("k_attn_fwd<bf16,16>", "k_attn_bwd<bf16,16>") and R.core_kernel("bf16", 4, 97, 1)[1] == "k_attn_bwd_2p32<4>"
    assert R.core_kernel("fp32", 2, 157, 1) == ("k_attn_fwd<float,64>", "k_attn_bwd<float,64>")
    # k_attn_bwd<float, 64> at T = 157: its LDS (one head at a time) is the 160 KB the launcher allows, and T = 158 is not
    lds = lambda L, hp, d: (4 * L * hp * d + L * hp * 4) * 4
    assert lds(157, 1, 64) <= 160 * 1024 < lds(158, 1, 64)


def test_block_plants():
    for bone, mode, B, T in ((0, 1, 31, 32), (1, 0, 1025, 1), (0, 1, 1, 4)):
        i = R.block_inputs(bone, mode, B, T)
        groups, L = R.n_groups(B, T, mode), R.group_len(T, mode)
        rows = sorted(r for v in i["where"].values() for r in v)
        want = sorted({R.token_of(G, (L - 1 - p) if (G == groups - 1 and G > 0) else p, T, mode) for G in R.planted_groups(bone, B, T, mode) for p in range(min(5, L))})
        per = R.wg_walks(groups, R.block_grid(bone, B, T, mode)[1])[0]
        assert rows == want and len(R.planted_groups(bone, B, T, mode)) == (3 if per > 1 else min(groups, 2))
        ref = R.block_ref(R.stored(i, "bf16"), B, T, mode)
        assert bool((ref["q"][:, 48:64] == 0).all()) and bool((ref["k"][:, 64:80] == 0).all())              # zero queries (head 3), equal keys (head 4)
        assert float(ref["v"][:, 80:96].abs().max()) > 50 * float(ref["v"][:, 96:112].abs().max())         # v x 100 (head 5)
        s = R._scores(R.to_groups(ref["q"], B, T, mode), R.to_groups(ref["k"], B, T, mode), 8)
        if L > 4:
            assert float(s[:, 2].max()) > 88.8                                                             # offset (head 2): past fp32's exp range
        assert float(s[:, 1].std()) > 16                                                                   # peaked (head 1)
        assert all(torch.isfinite(v).all() for v in ref.values())
