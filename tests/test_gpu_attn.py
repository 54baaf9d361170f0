"""The attention cores, the fused-d_o backward kernels and the fused attention-block forward on their own (include/kasf.h: kasf_op_attention_fwd / _bwd [_heads],
kasf_op_attention_bwd_fused_do, kasf_op_attn_block_fwd) against fp64 torch math of the same operation on the dtype-rounded operands (tests/attn_ref.py).
tests/test_gpu_ops.py keeps its own, older checks of the same entries.

How every comparison is set up:
  * Operands are built on the CPU from a fixed seed and rounded to the storage dtype; the reference is fp64 on what the device holds.  The heads of a case carry the
    plants of attn_ref.plant_qkv, one per head: peaked (a one-hot softmax), offset (scores beyond fp32's exp range), zero queries, equal keys, v x 100.  Forward cases
    carry the strong forms; backward cases the mild ones (attn_ref.fwd_level / bwd_level: softer for groups under 8 positions and for the kt kernels), plus one strong run per case in which dv is held and dq / dk need only be finite.
    The block forward is planted through the weight rows of a head, and through the LayerNorm plants of dense_ref on rows of x / x_limb.
  * Token-major operands have 64 rows of NaN behind row M and NaN in the gap columns of a padded leading dimension.  Outputs hold the sentinel 7 in rows >= M and in
    gap columns, and buffers a call must not write (lse_save for groups <= 32) hold it throughout: all of that must be there bit for bit afterwards.
  * Every case runs twice from identical inputs and must give the same bits.
  * o, dq, dk, dv and the saved q | k | v | o are judged per (token, head): the error of the head's 16-channel slice over the largest |ref| of that (group, head) block
    (the group's largest over all heads where the block is analytically zero: dk under zero queries, dq under equal keys); x_mid per row; lse as |got - ref| /
    max(1, |ref|).  bf16 outputs: the excess over the output's own ulp 2^-8 |ref|.  Bars: attn_ref.BAR32 / c16, none from a device run.
  * The block forward is judged stage by stage: q | k | v against LN + GEMM of x; o and lse against the core on the q | k | v THE DEVICE STORED; x_mid against the
    projection of the o the device stored (attn_ref.block_ref says why).  Evaluation mode (no saves) must give the training run's x_mid bit for bit.

Instantiations by test id (attn_ref.core_kernel, fused_do_grid and block_grid restate the dispatch; tests/test_attn_ops_cpu.py holds them to the tables):
  test_core          bf16 h8: T <= 32 -> k_attn_fwd_mfma<1> / k_attn_bwd_mfma<1>;  33..96 -> <3> / k_attn_bwd_long<3>;  97..128, ..192, ..256 -> <4 / 6 / 8> / k_attn_bwd_2p<4 / 6 / 8>;
                     T = 257 -> the LDS-resident k_attn_fwd / k_attn_bwd<bf16, 16>;  h4: k_attn_fwd_mfma32 / k_attn_bwd_2p32<1 / 3 / 4 / 6 / 8>;  h2 / h16 and fp32 mode:
                     k_attn_fwd / k_attn_bwd<T, 64 / 8 / ...>;  "bone": q at ld 128 apart from k | v at ld 256;  "+8": padded leading dimensions
  test_fused_do      pers9 / pers16 -> k_attn_bwd_pers<9 / 16> (form 1: k_attn_bwd_mfma<1, true>, bit-equal);  long -> k_attn_bwd_long<3, true>;  kt16 / kt9 -> k_attn_bwd_kt<3, 16 / 9>
  test_block         flat / rp / rp3 -> k_attn_blk_fwd_flat / _rp / _rp3 <BONE = false / true>
  test_handover      rp3 -> kt, rp -> pers<16>, flat -> pers<9>: the forward's own q | k | v (o, lse) into the backward
  test_isolation     one case per kernel above: the groups kept must not see the groups redrawn
  test_block_bwd     (kasf_op_attn_block_bwd) spatial and t9 -> k_attn_blk_bwd_h<BONE, 9>;  t16 -> <BONE, 16>;  then k_wgrad_ring_jobs + k_wgrad_finish_jobs
                     (ext job) and k_col_finish.  Stage by stage as test_block: LN(x) from x; dq | dk | dv and the proj gradients on the stored LN(x); out, out_limb, the
                     LayerNorm parameter gradients and dw on the stored dq | dk | dv.  test_block_bwd_short_sink: error 6;  test_block_bwd_isolation: three shapes per form
"""
import pytest
import torch

from tests import attn_ref as R
from tests.gpu_util import DT, stream

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
PAD = 64
F64 = torch.float64
NAN = float("nan")


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


def _in(cols, ld, dtype):
    """token-major operands side by side in one [M + PAD, ld] device buffer; NaN behind row M and in the gap columns"""
    M = cols[0].shape[0]
    d = torch.full((M + PAD, ld), NAN, dtype=dtype)
    c0 = 0
    for c in cols:
        d[:M, c0:c0 + c.shape[1]] = c.to(dtype)
        c0 += c.shape[1]
    return _dev(d, dtype)


def _out(M, ld, dtype):
    d = torch.full((M + PAD, ld), SENTINEL, device="cuda", dtype=dtype)
    _KEEP.append(d)
    return d


def _kept(buf, M, width, what):
    assert bool((buf[M:] == SENTINEL).all()), f"{what}: rows >= M were written"
    assert bool((buf[:M, width:] == SENTINEL).all()), f"{what}: the gap columns of the padded leading dimension were written"


def _ok(rc, lib):
    assert rc == 0, (rc, lib.kasf_last_error())
    torch.cuda.synchronize()


def _at(buf, col):
    return buf.data_ptr() + col * buf.element_size()


class Log:
    def __init__(self, tag, cd):
        self.tag, self.cd, self.lines, self.ok = tag, cd, [], True

    def add(self, name, e, bar, at=""):
        self.lines.append(f"{name} {e:.2e}{' at ' + str(at) if at != '' else ''} (bar {bar:.1e})")
        self.ok &= e <= bar

    def heads(self, key, name, got, ref, geom, H=8, zero=None):
        """a [M, 128] output per (token, head); bf16 mode: the excess over the output's own ulp"""
        mode, B, T = geom
        e, at = R.head_err(R.to_groups(got, B, T, mode), R.to_groups(ref, B, T, mode), H, zero, excess=self.cd == "bf16")
        self.add(name + (" excess" if self.cd == "bf16" else ""), e, R.bar(key, self.cd), at)

    def finite(self, name, got):
        self.lines.append(f"{name} finite")
        self.ok &= bool(torch.isfinite(got).all())

    def done(self):
        print(f"\n[attn {self.tag}] " + "; ".join(self.lines))
        assert self.ok, f"{self.tag}: " + "; ".join(self.lines)


def _same(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs between two runs from identical inputs"


def _twice(fn, what):
    a, b = fn(), fn()
    _same(a, b, what)
    return a


# ================================================================================================ the launches
def _qkv_buffers(i, dt, bone, pad, maker, names=("q", "k", "v")):
    """packed: q | k | v in one buffer of ld 384 (+ pad); bone: q at ld 128 (+ pad) apart from k | v at ld 256 (+ pad) -> (buffers, (q, ldq, k, v, ldkv) arguments)"""
    if bone:
        a, b = maker([i[names[0]]], 128 + pad, dt), maker([i[names[1]], i[names[2]]], 256 + pad, dt)
        return (a, b), (_at(a, 0), 128 + pad, _at(b, 0), _at(b, 128), 256 + pad)
    a = maker([i[n] for n in names], 384 + pad, dt)
    return (a,), (_at(a, 0), 384 + pad, _at(a, 128), _at(a, 256), 384 + pad)


def _grad_buffers(M, dt, bone, pad):
    if bone:
        a, b = _out(M, 128 + pad, dt), _out(M, 256 + pad, dt)
        return (a, b), (_at(a, 0), 128 + pad, _at(b, 0), _at(b, 128), 256 + pad)
    a = _out(M, 384 + pad, dt)
    return (a,), (_at(a, 0), 384 + pad, _at(a, 128), _at(a, 256), 384 + pad)


def _grads_back(bufs, M, what):
    for b in bufs:
        _kept(b, M, b.shape[1] // 128 * 128, what)
    t = torch.cat([b[:M, :b.shape[1] // 128 * 128] for b in bufs], dim=1).double().cpu()
    return dict(dq=t[:, :128], dk=t[:, 128:256], dv=t[:, 256:])


def run_core(lib, cd, H, geom, i, bone=False, pad=0, fwd=True, bwd=True):
    mode, B, T = geom
    code, dt = DT[cd]
    M = B * T * 17
    out = {}
    _, qargs = _qkv_buffers(i, dt, bone, pad, _in)
    if fwd:
        o = _out(M, 128, dt)
        _ok(lib.kasf_op_attention_fwd_heads(code, *qargs, o.data_ptr(), B, T, mode, H, stream()), lib)
        _kept(o, M, 128, "o")
        out["o"] = o[:M].double().cpu()
    if bwd:
        d_o = _in([i["d_o"]], 128, dt)
        gb, gargs = _grad_buffers(M, dt, bone, pad)
        _ok(lib.kasf_op_attention_bwd_heads(code, *qargs, d_o.data_ptr(), gargs[0], gargs[1], gargs[2], gargs[3], gargs[4], B, T, mode, H, stream()), lib)
        out.update(_grads_back(gb, M, "dq | dk | dv"))
    return out


def run_fused(lib, geom, i, bone=False, form=0, stats=None, pad=0):
    """stats: (o [M, 128] bf16 values, lse [M, 8]) token-major, or device buffers of the forward (hand-over)"""
    mode, B, T = geom
    dt = torch.bfloat16
    M = B * T * 17
    if "dev" in i:
        qargs = i["dev"]
    else:
        _, qargs = _qkv_buffers(i, dt, bone, pad, _in)
    g_mid, wts = _in([i["g_mid"]], 128, dt), _dev(i["wts"], dt)
    o = lse = None
    if stats is not None:
        o, lse = (stats if stats[0].is_cuda else (_in([stats[0]], 128, dt), _in([stats[1]], 8, torch.float32)))
    gb, gargs = _grad_buffers(M, dt, bone, pad)
    _ok(lib.kasf_op_attention_bwd_fused_do(*qargs, g_mid.data_ptr(), wts.data_ptr(), *gargs, B, T, mode, form, o.data_ptr() if o is not None else None,
                                           lse.data_ptr() if lse is not None else None, stream()), lib)
    return _grads_back(gb, M, "dq | dk | dv")


def run_block(lib, bone, geom, i, train=True, keep=None):
    """-> x_mid (, q, k, v, o, lse) as fp64 CPU tensors; keep: a dict that receives the device buffers of the saves (hand-over)"""
    mode, B, T = geom
    dt = torch.bfloat16
    M = B * T * 17
    x, xl = _in([i["x"]], 128, dt), (_in([i["xl"]], 128, dt) if bone else None)
    f = lambda n: _dev(i[n]).data_ptr() if i[n] is not None else None
    w = lambda n: _dev(i[n], dt).data_ptr() if i[n] is not None else None
    out = _out(M, 128, dt)
    q, kv, o, lse = _out(M, 128 if bone else 384, dt), _out(M, 256, dt), _out(M, 128, dt), _out(M, 8, torch.float32)
    p = lambda t, on=True: t.data_ptr() if (train and on) else None
    _ok(lib.kasf_op_attn_block_fwd(bone, x.data_ptr(), xl.data_ptr() if bone else None, f("ln_g"), f("ln_b"), f("lnl_g"), f("lnl_b"), w("wq"), w("wkv"), w("wproj"), f("bproj"),
                                   f("ls1"), p(q), p(kv, bone), p(o), p(lse), out.data_ptr(), B, T, mode, stream()), lib)
    _kept(out, M, 128, "x_mid")
    res = dict(x_mid=out[:M].double().cpu())
    rp3 = R.group_len(T, mode) > 32
    if not train:
        for n, b in (("q_save", q), ("kv_save", kv), ("o_save", o), ("lse_save", lse)):
            assert bool((b == SENTINEL).all()), f"{n} was written in evaluation mode"
        return res
    for n, b in (("q_save", q), ("o_save", o)) + ((("kv_save", kv),) if bone else ()) + ((("lse_save", lse),) if rp3 else ()):
        _kept(b, M, b.shape[1], n)
    if not bone:
        assert bool((kv == SENTINEL).all()), "kv_save was written by the self-attention form"
    if not rp3:
        assert bool((lse == SENTINEL).all()), "lse_save was written for groups of at most 32 positions"
    qkv = torch.cat((q[:M], kv[:M]), dim=1).double().cpu() if bone else q[:M].double().cpu()
    res.update(q=qkv[:, :128], k=qkv[:, 128:256], v=qkv[:, 256:], o=o[:M].double().cpu())
    if rp3:
        res["lse"] = lse[:M].double().cpu()
    if keep is not None:
        keep.update(q=q, kv=kv, o=o, lse=lse)
    return res


# ================================================================================================ A. the cores
def _core_params():
    ps = [("bf16", H, m, B, T, bone, 0) for H, m, B, T in R.CORE_BF16 for bone in ((False, True) if H == 8 else (False,))]
    ps += [("fp32", H, m, B, T, False, 0) for H, m, B, T in R.CORE_FP32]
    ps += [("bf16", H, m, B, T, False, 8) for H, m, B, T in R.CORE_PADDED] + [("bf16", 8, 1, 2, 96, True, 8), ("fp32", 8, 1, 2, 27, False, 8)]
    return ps


def _core_id(p):
    cd, H, m, B, T, bone, pad = p
    return f"{cd}-h{H}-{'spatial' if m == 0 else 'temporal'}-B{B}-T{T}" + ("-bone" if bone else "") + ("+8" if pad else "")


@pytest.mark.parametrize("p", _core_params(), ids=_core_id)
def test_core(lib, p):
    cd, H, mode, B, T, bone, pad = p
    geom = (mode, B, T)
    fk, bk = R.core_kernel(cd, H, T, mode)
    log = Log(f"core {_core_id(p)} [{fk} / {bk}]", cd)
    L = R.group_len(T, mode)
    fl, bl = R.fwd_level(L), R.bwd_level(L)
    i = R.stored(R.core_inputs(H, mode, B, T, fl), cd)
    ref = R.core_eval(i, H, mode, B, T)
    got = _twice(lambda: run_core(lib, cd, H, geom, i, bone, pad), log.tag)
    back = lambda n: R.from_groups(ref[n], B, T, mode)
    log.heads("core_fwd.o", f"o[{fl}]", got["o"], back("o"), geom, H)
    if L == 1:                                                 # one position: P = 1 exactly
        assert torch.equal(got["o"], i["v"].double()) and torch.equal(got["dv"], i["d_o"].double()), f"{log.tag}: o == v and dv == d_o bit for bit at one position"
        if H == 8:
            assert bool((got["dq"] == 0).all()) and bool((got["dk"] == 0).all()), f"{log.tag}: dq == dk == 0 at one position"
        else:
            # k_attn_bwd_2p32 forms delta = <o, d_o> apart from dP = <d_o, v>: dS = (dP - delta) / sqrt(d) is a rounding residue, not 0.  The reference is 0, so
            # the error has no |ref| to stand over: it is held against what dS multiplies, max |dP| / sqrt(d) x max |k| (dq; max |q| for dk), at the outputs' bar
            d = 128 // H
            dP = (i["d_o"].double() * i["v"].double()).reshape(-1, H, d).sum(-1).abs().max()
            for n, other in (("dq", "k"), ("dk", "q")):
                log.add(f"{n} (reference 0) over max|dP| |{other}| / sqrt(d)", float(got[n].abs().max() / (dP * d ** -0.5 * i[other].abs().max())), R.bar(f"core_bwd.{n}", cd))
    else:
        log.heads("core_bwd.dv", f"dv[{fl}]", got["dv"], back("dv"), geom, H)
        log.finite(f"dq[{fl}]", got["dq"])
        log.finite(f"dk[{fl}]", got["dk"])
        i = R.stored(R.core_inputs(H, mode, B, T, bl), cd)
        ref = R.core_eval(i, H, mode, B, T)
        got = _twice(lambda: run_core(lib, cd, H, geom, i, bone, pad, fwd=False), log.tag)
        for n in ("dq", "dk", "dv"):
            log.heads(f"core_bwd.{n}", f"{n}[{bl}]", got[n], back(n), geom, H, i["zero"].get(n))
    log.done()


# ================================================================================================ B. fused-d_o backward
def _fused_params():
    return [(name, m, B, T, bone) for name, cases in R.FUSED_DO.items() for m, B, T in cases for bone in (False, True)]


@pytest.mark.parametrize("name,mode,B,T,bone", _fused_params(), ids=lambda v: str(int(v)) if isinstance(v, bool) else str(v))
def test_fused_do(lib, name, mode, B, T, bone):
    geom = (mode, B, T)
    kt = name.startswith("kt")
    op = "kt" if kt else "fused_do"
    assert R.fused_do_grid(B, T, mode, kt)[0] == name
    log = Log(f"fused_do {name} mode={mode} B={B} T={T} bone={int(bone)}", "bf16")
    for level, only_dv in ((R.bwd_level(R.group_len(T, mode), kt), False), ("mild" if kt else "strong", True)):
        i = R.stored(R.fused_inputs(mode, B, T, level), "bf16")
        ref = R.fused_eval(i, mode, B, T)
        stats = None
        if kt:
            o, lse = R.kt_stats(i, mode, B, T)
            stats = (R.from_groups(o, B, T, mode), R.from_groups(lse, B, T, mode))
        got = _twice(lambda: run_fused(lib, geom, i, bone, 0, stats), log.tag)
        if R.group_len(T, mode) <= 32:
            _same(got, run_fused(lib, geom, i, bone, 1), log.tag + ": form 1 against form 0")
        for n in ("dq", "dk", "dv"):
            if only_dv and n != "dv":
                log.finite(f"{n}[{level}]", got[n])
            else:
                log.heads(f"{op}.{n}", f"{n}[{level}]", got[n], R.from_groups(ref[n], B, T, mode), geom, 8, i["zero"].get(n))
    log.done()


# ================================================================================================ C. the block forward
def _judge_block(log, i, geom, got, x_mid_only=False):
    mode, B, T = geom
    given = {n: got[n] for n in ("q", "k", "v", "o")}
    ref = R.block_ref(i, B, T, mode, given=given)
    for n in ("q", "k", "v", "o"):
        log.heads(f"block.{n}", n, got[n], ref[n], geom)
    if "lse" in got:
        log.add("lse", R.lse_err(got["lse"], ref["lse"]), R.bar("block.lse", "bf16"))
    e, row = R.row_excess(got["x_mid"], ref["x_mid"])
    log.add("x_mid excess", e, R.bar("block.x_mid", "bf16"), f"row {row}")


def _block_params():
    return [(name, m, B, T, bone) for name, cases in R.BLOCK.items() for m, B, T in cases for bone in (0, 1)]


@pytest.mark.parametrize("name,mode,B,T,bone", _block_params())
def test_block(lib, name, mode, B, T, bone):
    geom = (mode, B, T)
    assert R.block_grid(bone, B, T, mode)[0] == name
    log = Log(f"block {name} mode={mode} B={B} T={T} bone={bone} [k_attn_blk_fwd_{name}<{'true' if bone else 'false'}>]", "bf16")
    i = R.stored(R.block_inputs(bone, mode, B, T), "bf16")
    got = _twice(lambda: run_block(lib, bone, geom, i, True), log.tag)
    ev = _twice(lambda: run_block(lib, bone, geom, i, False), log.tag + " evaluation")
    assert torch.equal(ev["x_mid"], got["x_mid"]), f"{log.tag}: x_mid differs between training (saves given) and evaluation (saves NULL)"
    _judge_block(log, i, geom, got)
    log.done()


@pytest.mark.parametrize("bone", [0, 1])
def test_block_flat_long_walk(lib, bone):
    """49 frames in workgroup 0: every rolling offset (17 j) mod 48 of the q | k | v tiles, both tile parities, all three hb (training mode only)"""
    mode, B, T = geom = R.BLOCK_LONG[bone]
    assert R.wg_walks(B, R.block_grid(bone, B, T, mode)[1])[0] == 49
    log = Log(f"block flat long frames={B} bone={bone}", "bf16")
    i = R.stored(R.block_inputs(bone, mode, B, T), "bf16")
    got = _twice(lambda: run_block(lib, bone, geom, i, True), log.tag)
    _judge_block(log, i, geom, got)
    log.done()


# ================================================================================================ D. hand-over, forward to backward
@pytest.mark.parametrize("bone", [0, 1])
@pytest.mark.parametrize("mode,B,T", R.HANDOVER)
def test_handover(lib, mode, B, T, bone):
    geom = (mode, B, T)
    fwd, bwd = R.block_grid(bone, B, T, mode)[0], R.fused_do_grid(B, T, mode, True)[0]
    kt = bwd.startswith("kt")
    op = "kt" if kt else "fused_do"
    log = Log(f"handover {fwd} -> {bwd} mode={mode} B={B} T={T} bone={bone}", "bf16")
    bi = R.stored(R.block_inputs(bone, mode, B, T, "none"), "bf16")          # (no peaked or offset head: attn_ref.measure says what the reference carries here)
    dev = {}
    f = run_block(lib, bone, geom, bi, True, keep=dev)
    fi = R.stored(R.fused_inputs(mode, B, T, "faint"), "bf16")
    i = dict(q=f["q"], k=f["k"], v=f["v"], g_mid=fi["g_mid"], wts=fi["wts"])
    q, kv = dev["q"], dev["kv"]
    i["dev"] = (_at(q, 0), 128, _at(kv, 0), _at(kv, 128), 256) if bone else (_at(q, 0), 384, _at(q, 128), _at(q, 256), 384)
    got = _twice(lambda: run_fused(lib, geom, i, bone, 0, (dev["o"], dev["lse"]) if kt else None), log.tag)
    ref = R.fused_eval(i, mode, B, T)
    zero = R.handover_zero(B, T, mode)
    for n in ("dq", "dk", "dv"):
        log.heads(f"{op}.{n}", n, got[n], R.from_groups(ref[n], B, T, mode), geom, 8, zero.get(n))
    if kt:                                                    # and against the self-contained kernel on the same operands (o / lse NULL)
        alone = run_fused(lib, geom, i, bone, 0, None)
        for n in ("dq", "dk", "dv"):
            log.heads(f"kt.{n}", f"{n} against k_attn_bwd_long", got[n], alone[n], geom, 8, zero.get(n))
    log.done()


# ================================================================================================ E. isolation
def _mix(a, b, geom):
    """rows of the groups with index divisible by 3 from a, every other group's from b -> (mixed, kept rows mask [M])"""
    mode, B, T = geom
    ga, gb = R.to_groups(a, B, T, mode), R.to_groups(b, B, T, mode)
    keep = torch.arange(ga.shape[0]) % 3 == 0
    mixed = torch.where(keep[:, None, None], ga, gb)
    rows = R.from_groups(keep[:, None, None].expand(-1, ga.shape[1], 1).double(), B, T, mode)[:, 0] > 0
    return R.from_groups(mixed, B, T, mode), rows


def _redraw(i, names, geom, seed):
    g = R.gen(77, seed)
    j, rows = dict(i), None
    for n in names:
        if i.get(n) is not None:
            j[n], rows = _mix(i[n], torch.randn(i[n].shape, generator=g).to(torch.bfloat16).float(), geom)
    return j, rows


ISOLATION = [("core", "bf16", 8, 0, 3, 27), ("core", "bf16", 8, 1, 2, 27), ("core", "bf16", 8, 1, 2, 81), ("core", "bf16", 8, 1, 2, 128), ("core", "bf16", 8, 1, 2, 257),
             ("core", "bf16", 4, 1, 2, 33), ("core", "bf16", 4, 0, 3, 27), ("core", "fp32", 8, 0, 3, 27), ("core", "fp32", 2, 1, 2, 27)] + \
            [("fused", name, 0, *c) for name, c in (("pers9", (0, 41, 27)), ("pers16", (1, 31, 32)), ("long", (1, 2, 65)), ("kt16", (1, 3, 96)), ("kt9", (1, 3, 81)))] + \
            [("block", name, bone, *c) for name, c in (("flat", (0, 1025, 1)), ("rp", (1, 31, 32)), ("rp3", (1, 16, 81))) for bone in (0, 1)]


@pytest.mark.parametrize("case", ISOLATION, ids=lambda c: "-".join(str(v) for v in c))
def test_isolation(lib, case):
    """a group's result must not depend on any other group: the groups with index not divisible by 3 are redrawn (finite values), the others' outputs keep their bits"""
    kind, a, b, mode, B, T = case
    geom = (mode, B, T)
    if kind == "core":
        i = R.stored(R.core_inputs(b, mode, B, T, "mild"), a)
        run = lambda i: run_core(lib, a, b, geom, i)
        names = ("q", "k", "v", "d_o")
    elif kind == "fused":
        kt = a.startswith("kt")
        i = R.stored(R.fused_inputs(mode, B, T, "faint"), "bf16")

        def run(i):
            stats = None
            if kt:
                o, lse = R.kt_stats(i, mode, B, T)
                stats = (R.from_groups(o, B, T, mode), R.from_groups(lse, B, T, mode))
            return run_fused(lib, geom, i, False, 0, stats)
        names = ("q", "k", "v", "g_mid")
    else:
        i = R.stored(R.block_inputs(b, mode, B, T), "bf16")
        run = lambda i: run_block(lib, b, geom, i, True)
        names = ("x", "xl")
    j, rows = _redraw(i, names, geom, 1)
    first, second = run(i), run(j)
    changed = 0
    for n in first:
        assert torch.equal(first[n][rows], second[n][rows]), f"{case}: {n} of a kept group changed when other groups were redrawn"
        changed += int((first[n][~rows] != second[n][~rows]).sum())
    assert changed > 0, f"{case}: the redrawn groups' outputs did not change"


# ================================================================================================ F. block backward
WPROJ_BYTES = 256 * 128 * 128 * 2 + 256 * 128 * 4
BWD_ACC = ("dgamma", "dbeta", "dgamma_l", "dbeta_l", "dw_mix", "dw_kv", "dproj_w", "dproj_b", "dls1")


def run_block_bwd(lib, bone, geom, i, sink_rows=None, expect=0):
    """-> every output as fp64 CPU tensors (the accumulated fp32 ones with their start value 1 taken off); sink_rows: the rows of the column sink (default: the active
    workgroups).  Token-major operands carry 64 rows of NaN behind row M, written token-major outputs the sentinel; out_limb starts from random bf16 values; partial,
    proj_part and the sink start at NaN with a NaN guard behind the size the entry is told."""
    from tests.dense_ref import jobs_splits
    mode, B, T = geom
    bf = torch.bfloat16
    M = B * T * 17
    x, g_mid = _in([i["x"]], 128, bf), _in([i["g_mid"]], 128, bf)
    xl = _in([i["xl"]], 128, bf) if bone else None
    f = lambda n: _dev(i[n]).data_ptr() if i.get(n) is not None else None
    w = lambda n, t=None: _dev(i[n] if t is None else t, bf).data_ptr() if i.get(n) is not None else None
    out, dq, xn_a = _out(M, 128, bf), _out(M, 128 if bone else 384, bf), _out(M, 128, bf)
    out_limb = dkv = xn_b = None
    if bone:
        dkv, xn_b = _out(M, 256, bf), _out(M, 128, bf)
        out_limb = _in([i["outl0"]], 128, bf)
        out_limb[M:] = SENTINEL
    acc = {n: torch.ones(s, device="cuda") for n, s in (("dgamma", 128), ("dbeta", 128), ("dw_mix", (128 if bone else 384, 128)), ("dproj_w", (128, 128)), ("dproj_b", 128),
                                                        ("dls1", 128))}
    if bone:
        acc.update({n: torch.ones(s, device="cuda") for n, s in (("dgamma_l", 128), ("dbeta_l", 128), ("dw_kv", (256, 128)))})
    need = jobs_splits(M, (128, 256) if bone else (384,))[0] * 384 * 128
    active = R.block_bwd_grid(B, T, mode)[2]
    sink = ((active if sink_rows is None else sink_rows) * (512 if bone else 256) + 63) // 64 * 64
    nan = lambda n, dt=torch.float32: torch.full((n + 64,), NAN, device="cuda", dtype=dt)
    partial, ppart, scratch = nan(need), nan(WPROJ_BYTES // 2, bf), nan(sink)
    _KEEP.extend([acc, partial, ppart, scratch])
    p = lambda t: t.data_ptr() if t is not None else None
    a = lambda n: acc[n].data_ptr() if n in acc else None
    rc = lib.kasf_op_attn_block_bwd(bone, p(x), p(xl), p(g_mid), f("ln_g"), f("ln_b"), f("lnl_g"), f("lnl_b"), w("wq"), w("wkv"), w("wq", i["wq"].T.contiguous()) if bone else None,
                                    w("wts"), f("proj_w"), f("proj_b"), f("ls1"), p(out), p(out_limb), p(dq), p(dkv), p(xn_a), p(xn_b), a("dgamma"), a("dbeta"),
                                    a("dgamma_l"), a("dbeta_l"), a("dw_mix"), a("dw_kv"), a("dproj_w"), a("dproj_b"), a("dls1"), p(partial), need, p(ppart), WPROJ_BYTES,
                                    p(scratch), sink, B, T, mode, stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.kasf_last_error())
    for n, b in (("partial", partial[need:]), ("proj_part", ppart[WPROJ_BYTES // 2:]), ("scratch", scratch[sink:])):
        assert bool(torch.isnan(b).all()), f"the guard behind {n} was written"
    toks = dict(out=out, dq=dq, xn=xn_a, **(dict(out_limb=out_limb, dkv=dkv, xnl=xn_b) if bone else {}))
    if expect != 0:                                            # refused or declined: nothing was launched, every buffer keeps its start value
        assert all(bool((t == SENTINEL).all()) for n, t in toks.items() if n != "out_limb") and all(bool((t == 1).all()) for t in acc.values())
        assert bool(torch.isnan(partial).all()) and bool(torch.isnan(ppart).all()) and bool(torch.isnan(scratch).all())
        return None
    for n, t in toks.items():
        _kept(t, M, t.shape[1], n)
    res = {n: t[:M].double().cpu() for n, t in toks.items() if n not in ("dq", "dkv")}
    d = torch.cat((dq[:M], dkv[:M]), dim=1).double().cpu() if bone else dq[:M].double().cpu()
    res.update(dq=d[:, :128], dk=d[:, 128:256], dv=d[:, 256:])
    res.update({n: t.double().cpu() - 1 for n, t in acc.items()})
    return res


def _bwd_params():
    return [(name, m, B, T, bone) for name, cases in R.BLOCK_BWD.items() for m, B, T in cases for bone in (0, 1)]


def _bwd_judge(log, got, ref, geom, names):
    """one stage's outputs in their measures: dq | dk | dv per (token, head), the token-major ones per row over their own bf16 ulp, the reductions per tensor (+ one
    fp32 addition into the buffer that held 1)"""
    from tests.dense_ref import rel_err
    zero = R.handover_zero(geom[1], geom[2], geom[0])
    for stage, outs in R.BWD_STAGES.items():
        for n in outs:
            if n not in names or n not in ref:
                continue
            key = f"bwd.{stage}"
            if n in ("dq", "dk", "dv"):
                log.heads(key, n, got[n], ref[n], geom, 8, zero.get(n))
            elif n in ("xn", "xnl", "out", "out_limb"):
                e, row = R.row_excess(got[n], ref[n])
                log.add(f"{n} excess", e, R.bar(key, "bf16"), f"row {row}")
            else:
                mx = max(float(ref[n].abs().max()), 1e-300)
                log.add(n, rel_err(got[n], ref[n]), R.bar(key, "bf16") + 2.0 ** -24 * (1 + mx) / mx)


@pytest.mark.parametrize("name,mode,B,T,bone", _bwd_params(), ids=lambda v: str(v))
def test_block_bwd(lib, name, mode, B, T, bone):
    """kasf_launch_attn_block_bwd + the streaming weight gradient with its ext job + the sink's flush, stage by stage against attn_ref.block_bwd_ref: LN(x) from x;
    dq | dk | dv on the LN(x) the device stored; out, out_limb, the LayerNorm parameter gradients and dw_mix / dw_kv on the dq | dk | dv (and LN(x)) it stored; the
    proj gradients from the stored LN(x) (o is never stored)"""
    geom = (mode, B, T)
    i = R.stored(R.block_bwd_inputs(bone, mode, B, T), "bf16")
    grid, per, active = R.block_bwd_grid(B, T, mode)
    log = Log(f"block_bwd {name} mode={mode} B={B} T={T} bone={bone} [k_attn_blk_bwd_h<{bool(bone)}, {9 if R.group_len(T, mode) <= 17 else 16}>, per {per}, active {active}]", "bf16")
    got = _twice(lambda: run_block_bwd(lib, bone, geom, i), log.tag)
    _bwd_judge(log, got, R.block_bwd_ref(i, B, T, mode), geom, ("xn", "xnl"))
    want = i["ln_b"].to(torch.bfloat16).double()
    for r in i["where"]["const"] + i["where"]["zero"]:
        assert torch.equal(got["xn"][r], want), f"{log.tag}: LN of the planted constant row {r} is not beta exactly"
    st = {n: got[n] for n in ("xn", "xnl") if n in got}
    _bwd_judge(log, got, R.block_bwd_ref(i, B, T, mode, given=st), geom, ("dq", "dk", "dv", "dproj_w", "dls1", "dproj_b"))
    st.update({n: got[n] for n in ("dq", "dk", "dv")})
    _bwd_judge(log, got, R.block_bwd_ref(i, B, T, mode, given=st), geom, ("out", "out_limb", "dgamma", "dbeta", "dgamma_l", "dbeta_l", "dw_mix", "dw_kv"))
    log.done()


@pytest.mark.parametrize("bone", [0, 1])
def test_block_bwd_short_sink(lib, bone):
    """the column sink one row short of the active workgroups: error 6, nothing launched, every buffer untouched; with the full sink the same call runs"""
    geom = (1, 16, 17)
    i = R.stored(R.block_bwd_inputs(bone, *geom), "bf16")
    active = R.block_bwd_grid(16, 17, 1)[2]
    assert run_block_bwd(lib, bone, geom, i, sink_rows=active - 1, expect=6) is None
    assert run_block_bwd(lib, bone, geom, i) is not None


@pytest.mark.parametrize("mode,B,T,bone", [(m, B, T, bone) for m, B, T in ((0, 513, 1), (1, 31, 32), (1, 16, 17)) for bone in (0, 1)], ids=lambda v: str(v))
def test_block_bwd_isolation(lib, mode, B, T, bone):
    """the groups with index not divisible by 3 redrawn (x, x_limb, g_mid): the token-major outputs of the other groups keep their bits"""
    geom = (mode, B, T)
    i = R.stored(R.block_bwd_inputs(bone, mode, B, T), "bf16")
    j, rows = _redraw(i, ("x", "xl", "g_mid"), geom, 2)
    first, second = run_block_bwd(lib, bone, geom, i), run_block_bwd(lib, bone, geom, j)
    changed = 0
    for n in ("xn", "xnl", "dq", "dk", "dv", "out", "out_limb"):
        if n in first:
            assert torch.equal(first[n][rows], second[n][rows]), f"block_bwd {geom} bone={bone}: {n} of a kept group changed when other groups were redrawn"
            changed += int((first[n][~rows] != second[n][~rows]).sum())
    assert changed > 0
