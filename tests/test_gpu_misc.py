"""The prologue, gate, head and embedding kernels on their own (include/kasf.h: kasf_op_prologue_fwd ... kasf_op_add; csrc/k_misc.hip and the fixed-order finish
k_col_finish of csrc/k_reduce.hip) against fp64 torch math of the same operation on the dtype-rounded operands (tests/misc_ref.py).

How every comparison is set up:
  * Operands are built on the CPU from a fixed seed and rounded to the storage dtype; the reference is fp64 on what the device holds.
  * Buffers that are written start at a sentinel; buffers that are accumulated into (dw, db, dpos, dls, the flat grads) start at 1.
  * Every op with a scratch argument runs with scratch (one row per workgroup + k_col_finish) and without (fp32 atomics); every scratch case runs twice from
    identical inputs and must give the same bits.
  * fp32 outputs -- bone3, limb3, alpha, head out, din3 and ALL weight / bias / position gradients, in both dtypes -- take the op's fp32 bar (misc_ref.BAR32: 8 x the
    measured error of a plain fp32 evaluation of the reference), each tensor by rel_err against its own largest value: no cosine, no pooling.
    An output that is accumulated into a buffer holding 1 also carries the rounding of every fp32 addition INTO that buffer, 2^-24 (1 + |ref|max) each, which is
    added to its bar: ONE addition with scratch (k_col_finish sums the rows, then `dst += v` once), and one per workgroup of the launch without (each workgroup's
    atomicAdd lands on the element that holds 1, in an order that changes from run to run) -- `_adds` restates the launchers' grid sizes for that.
  * Outputs stored in the model dtype take, in bf16, per element |got - ref| <= 2^-8 |ref| + bar32 |ref|max (one bf16 ulp on top of the fp32 arithmetic).

k_col_finish row counts (one row per workgroup of the producer; 8 x 16 rows per unrolled pass, 16 per tail pass):
     1        every op at frames / M = 1
     2, 5     embed_bwd frames 2, 5 (gate / head M = 17: 2)
     15-17    embed_bwd frames 15, 16, 17
     50       refusion_bwd frames 50
     127-129  embed_bwd frames 127 (127), 128 (128); gate_bwd / head_bwd M = 2,033 (128), 2,049 (129)
     255-257  refusion_bwd frames 255 (255), 256 (256); head_bwd M = 4,099 (256, its cap); gate_bwd M = 4,099 (257)
     768      gate_bwd M = 12,291 and 30,011 (its cap)
"""
import ctypes as C

import pytest
import torch

from tests import misc_ref as R
from tests.gpu_util import DT, ptr, stream

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
J = 17
CDS = ["fp32", "bf16"]
SCRATCH = [True, False]


@pytest.fixture(scope="module")
def lib():
    from kasportsformer_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def models(lib):
    """cd -> (handle of a one-layer model with its device tables, entries, flat fp32 parameters on the device, name -> fp64 CPU tensor)"""
    from kasportsformer_amd import _lib
    made = {}

    def get(cd):
        if cd not in made:
            cfg, h = _lib.KasfConfig(1, 4, 8, 4, 1, DT[cd][0]), C.c_void_p()
            _lib.check(lib.kasf_model_create(C.byref(cfg), C.byref(h)))
            ents = _lib.param_entries(h)
            flat = R.fill_params(ents, lib.kasf_param_count(h))
            made[cd] = (h, ents, flat.cuda(), R.named(flat, ents, torch.float64))
        return made[cd]

    yield get
    torch.cuda.synchronize()
    for h, *_ in made.values():
        lib.kasf_model_destroy(h)


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


def _new(shape, dtype=torch.float32, fill=SENTINEL):
    d = torch.full(shape if isinstance(shape, tuple) else (shape,), fill, device="cuda", dtype=dtype)
    _KEEP.append(d)
    return d


def _back(t):
    return t.detach().double().cpu()


def _scratch(lib, op, n, use, short=0):
    """(device scratch or None, its size in floats); short: that many floats fewer than the op asks for"""
    if not use:
        return None, 0
    need = lib.kasf_op_misc_scratch_floats(op, n)
    assert need > 0 and need % 64 == 0
    return _new(need, fill=float("nan")), need - short


def _ok(rc, lib):
    assert rc == 0, (rc, lib.kasf_last_error())
    torch.cuda.synchronize()


class Log:
    def __init__(self, tag):
        self.tag, self.lines, self.ok = tag, [], True

    def f32(self, name, got, ref, bar, adds=0):
        """an fp32 output: rel_err against its own largest value; adds: fp32 additions into the buffer (holding 1) that the output was accumulated into"""
        if adds:
            bar = bar + adds * 2.0 ** -24 * (1 + float(ref.abs().max())) / max(float(ref.abs().max()), 1e-300)
        e = R.rel_err(got, ref)
        self.lines.append(f"{name} {e:.2e} (bar {bar:.2e})")
        self.ok &= e <= bar
        return e

    def stored(self, name, got, ref, cd, bar):
        """an output stored in the model dtype"""
        if cd == "fp32":
            return self.f32(name, got, ref, bar)
        mx = max(float(ref.abs().max()), 1e-300)
        e = float(((got - ref).abs() - 2.0 ** -8 * ref.abs()).max() / mx)
        self.lines.append(f"{name} excess over a bf16 ulp {e:.2e} (bar {bar:.2e})")
        self.ok &= e <= bar
        return e

    def done(self):
        print(f"\n[misc {self.tag}] " + "; ".join(self.lines))
        assert self.ok, f"{self.tag}: " + "; ".join(self.lines)


def _adds(op, n, use_scratch):
    """additions into one element of an accumulated output: 1 with scratch, else the workgroups of the launch (k_misc.hip: embed min(frames, 128), refusion
    min(frames, 256), gate and head one workgroup per 16 tokens, at most 256 on the atomics)"""
    if use_scratch:
        return 1
    return {"embed": min(n, 128), "refusion": min(n, 256), "gate": min((n + 15) // 16, 256), "head": min((n + 15) // 16, 256)}[op]


def _same_bits(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs between two runs from identical inputs"


# ================================================================================================ prologue
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("frames", R.PROLOGUE_FRAMES)
def test_prologue_fwd(lib, models, cd, frames):
    h, ents, flat, P = models(cd)
    dt, bar = DT[cd][1], R.BAR32["prologue"]
    x = R.prologue_x(frames)
    xd = _dev(x)
    outs = {n: _new((frames * J, 128), dt) for n in ("xj", "xb", "xl")}
    outs.update({n: _new((frames, J, 3)) for n in ("bone3", "limb3")})
    _ok(lib.kasf_op_prologue_fwd(h, ptr(flat), ptr(xd), ptr(outs["xj"]), ptr(outs["xb"]), ptr(outs["xl"]), ptr(outs["bone3"]), ptr(outs["limb3"]), frames,
                                 stream()), lib)
    ref = R.prologue_ref(x.double(), P)
    log = Log(f"prologue {cd} frames={frames}")
    for n in ("bone3", "limb3"):
        log.f32(n, _back(outs[n]), ref[n], bar)
    for n in ("xj", "xb", "xl"):
        log.stored(n, _back(outs[n]), ref[n], cd, bar)
    # the planted frames, exactly: a zero-length bone has length 1 and direction 0; an all-zero frame has that in every row, the mean row included
    b3 = outs["bone3"].cpu()
    assert b3[0, 2].tolist() == [0.0, 0.0, 1.0] and b3[0, 13].tolist() == [0.0, 0.0, 1.0]
    if frames >= 3:
        assert torch.equal(b3[2], torch.tensor([0.0, 0.0, 1.0]).expand(J, 3))
    if frames > 2050:
        assert b3[2048, 2].tolist() == [0.0, 0.0, 1.0] and torch.equal(b3[2050], torch.tensor([0.0, 0.0, 1.0]).expand(J, 3))
    log.done()


# ================================================================================================ embedding backward
def _run_embed(lib, cd, frames, use_scratch, with_din3, short=0):
    code, dt = DT[cd]
    i = R.embed_inputs(frames)
    g, in3, w = _dev(i["g"], dt), _dev(i["in3"]), _dev(i["w"])
    dw, db, dpos = _new((128, 3), fill=1.0), _new(128, fill=1.0), _new((J, 128), fill=1.0)
    din3 = _new((frames * J, 3)) if with_din3 else None
    sc, scn = _scratch(lib, 0, frames, use_scratch, short)
    rc = lib.kasf_op_embed_bwd(code, ptr(g), ptr(in3), ptr(w), ptr(dw), ptr(db), ptr(dpos), ptr(din3), frames, ptr(sc), scn, stream())
    torch.cuda.synchronize()
    out = dict(dw=dw.cpu(), db=db.cpu(), dpos=dpos.cpu())
    if with_din3:
        out["din3"] = din3.cpu()
    return rc, out, (_back(g), _back(in3), _back(w))


def _check_embed(log, out, ops, with_din3, adds):
    bar = R.BAR32["embed_bwd"]
    ref = R.embed_bwd_ref(*ops)
    for n in ("dw", "db", "dpos"):
        log.f32(n, out[n].double() - 1, ref[n], bar, adds=adds)
    log.f32("dpos[16]", out["dpos"][16].double() - 1, ref["dpos"][16], bar, adds=adds)      # the side path of k_embed_bwd (has16, two __shfl_xor steps), on its own
    if with_din3:
        log.f32("din3", out["din3"].double(), ref["din3"], bar)


@pytest.mark.parametrize("use_scratch", SCRATCH)
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("frames", R.EMBED_FRAMES)
def test_embed_bwd(lib, cd, frames, use_scratch):
    for with_din3 in (True, False):
        rc, out, ops = _run_embed(lib, cd, frames, use_scratch, with_din3)
        assert rc == 0, (rc, lib.kasf_last_error())
        log = Log(f"embed_bwd {cd} frames={frames} scratch={use_scratch} din3={with_din3}")
        _check_embed(log, out, ops, with_din3, _adds("embed", frames, use_scratch))
        log.done()
        if use_scratch:
            _same_bits(out, _run_embed(lib, cd, frames, True, with_din3)[1], log.tag)


# ================================================================================================ limb-refusion backward
def _run_refusion(lib, models, frames, use_scratch, short=0):
    h, ents, flat, P = models("fp32")           # k_refusion_bwd is fp32 throughout: the model's dtype takes no part
    i = R.refusion_inputs(frames)
    x, dl = _dev(i["x"]), _dev(i["dlimb3"])
    grads = _new(flat.numel(), fill=1.0)
    sc, scn = _scratch(lib, 1, frames, use_scratch, short)
    rc = lib.kasf_op_refusion_bwd(h, ptr(flat), ptr(x), ptr(dl), ptr(grads), frames, ptr(sc), scn, stream())
    torch.cuda.synchronize()
    return rc, grads.cpu()


def _check_refusion(log, models, frames, grads, adds):
    h, ents, flat, P = models("fp32")
    i = R.refusion_inputs(frames)
    ref = R.refusion_bwd_ref(i["x"].double(), i["dlimb3"].double(), P)
    assert len(ref) == 204
    untouched = torch.ones_like(grads, dtype=torch.bool)
    worst = (0.0, None)
    for n, off, s in ents:
        if n in ref:
            cnt = ref[n].numel()
            got = grads[off:off + cnt].double().view(ref[n].shape) - 1
            untouched[off:off + cnt] = False
            mx = float(ref[n].abs().max())
            bar = R.BAR32["refusion_bwd"] + adds * 2.0 ** -24 * (1 + mx) / max(mx, 1e-300)
            e = R.rel_err(got, ref[n])
            if e > bar:                                            # one by one: each of the 204 against its own largest value
                log.ok = False
                log.lines.append(f"{n} {e:.2e} (bar {bar:.2e})")
            if e / bar > worst[0]:
                worst = (e / bar, f"{n} {e:.2e} (bar {bar:.2e})")
    log.lines.append(f"worst of 204: {worst[1]}")
    # everything outside the 204 tensors -- the other parameters' gradients and the alignment gaps between the limb tensors -- still holds its start value exactly
    assert int(untouched.sum()) > 0 and bool((grads[untouched] == 1.0).all()), "refusion_bwd changed gradients outside the 204 limb-MLP tensors"


@pytest.mark.parametrize("use_scratch", SCRATCH)
@pytest.mark.parametrize("frames", R.REFUSION_FRAMES)
def test_refusion_bwd(lib, models, frames, use_scratch):
    rc, grads = _run_refusion(lib, models, frames, use_scratch)
    assert rc == 0, (rc, lib.kasf_last_error())
    log = Log(f"refusion_bwd frames={frames} scratch={use_scratch}")
    _check_refusion(log, models, frames, grads, _adds("refusion", frames, use_scratch))
    log.done()
    if use_scratch:
        assert torch.equal(grads, _run_refusion(lib, models, frames, True)[1]), f"{log.tag}: two runs from identical inputs differ"


# ================================================================================================ gate
def _gate_operands(cd, M, scale=1.0):
    dt = DT[cd][1]
    i = R.gate_inputs(M, scale)
    d = {n: _dev(i[n], dt) for n in ("xa", "xg", "xb", "g", "g1", "g2")}
    d["w"], d["bias"] = _dev(i["w"]), _dev(i["bias"])
    return d, {n: _back(t) for n, t in d.items()}


def _run_gate_fwd(lib, cd, M, d, adaptive):
    code, dt = DT[cd]
    out, alpha = _new((M, 128), dt), _new((M, 4))
    _ok(lib.kasf_op_gate_fwd(code, ptr(d["xa"]), ptr(d["xg"]), ptr(d["xb"]), ptr(d["w"]), ptr(d["bias"]), ptr(out), ptr(alpha), M, adaptive, stream()), lib)
    return out, alpha


@pytest.mark.parametrize("adaptive", [1, 0])
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("M", R.GATE_FWD_M)
def test_gate_fwd(lib, cd, M, adaptive):
    d, op = _gate_operands(cd, M)
    out, alpha = _run_gate_fwd(lib, cd, M, d, adaptive)
    ref = R.gate_fwd_ref(op["xa"], op["xg"], op["xb"], op["w"], op["bias"], adaptive)
    log = Log(f"gate_fwd {cd} M={M} adaptive={adaptive}")
    log.f32("alpha", _back(alpha[:, :3]), ref["alpha"], R.BAR32["gate_fwd"])
    log.stored("out", _back(out), ref["out"], cd, R.BAR32["gate_fwd"])
    assert bool((alpha[:, 3] == SENTINEL).all()), "alpha slot 3 is documented as not written"
    if not adaptive:
        assert bool((alpha[:, :3] == torch.tensor(1.0 / 3.0, dtype=torch.float32)).all())
    log.done()


def _run_gate_bwd(lib, cd, M, d, alpha, adaptive, extra, use_scratch, short=0):
    code, dt = DT[cd]
    ga, gg, gb = (_new((M, 128), dt) for _ in range(3))
    dw, db = _new((3, 384), fill=1.0), _new(3, fill=1.0)
    sc, scn = _scratch(lib, 2, M, use_scratch, short)
    rc = lib.kasf_op_gate_bwd(code, ptr(d["g"]), ptr(d["g1"]) if extra else None, ptr(d["g2"]) if extra else None, ptr(d["xa"]), ptr(d["xg"]), ptr(d["xb"]),
                              ptr(d["w"]), ptr(alpha), ptr(ga), ptr(gg), ptr(gb), ptr(dw), ptr(db), M, adaptive, ptr(sc), scn, stream())
    torch.cuda.synchronize()
    return rc, dict(ga=ga.cpu(), gg=gg.cpu(), gb=gb.cpu(), dw=dw.cpu(), db=db.cpu())


def _check_gate_bwd(log, cd, out, op, alpha, adaptive, extra, adds, v=""):
    bar = R.BAR32["gate_bwd"]
    g = op["g"] + op["g1"] + op["g2"] if extra else op["g"]
    ref = R.gate_bwd_ref(g, op["xa"], op["xg"], op["xb"], op["w"], _back(alpha[:, :3]), adaptive)
    for n in ("ga", "gg", "gb"):
        log.stored(v + n, out[n].double(), ref[n], cd, bar)
    if adaptive:
        log.f32(v + "dw", out["dw"].double() - 1, ref["dw"], bar, adds=adds)
        log.f32(v + "db", out["db"].double() - 1, ref["db"], bar, adds=adds)
    else:
        assert bool((out["dw"] == 1).all()) and bool((out["db"] == 1).all()), "adaptive = 0 must leave dw / db alone"
    return ref


@pytest.mark.parametrize("use_scratch", SCRATCH)
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("M", R.GATE_BWD_M)
def test_gate_bwd(lib, cd, M, use_scratch):
    d, op = _gate_operands(cd, M)
    log = Log(f"gate_bwd {cd} M={M} scratch={use_scratch}")
    for adaptive in (1, 0):
        _, alpha = _run_gate_fwd(lib, cd, M, d, adaptive)               # the stored alpha is an operand of the backward (compared in test_gate_fwd)
        for extra in (False, True):
            rc, out = _run_gate_bwd(lib, cd, M, d, alpha, adaptive, extra, use_scratch)
            assert rc == 0, (rc, lib.kasf_last_error())
            _check_gate_bwd(log, cd, out, op, alpha, adaptive, extra, _adds("gate", M, use_scratch), v=f"[a{adaptive} x{int(extra)}] ")
            if use_scratch:
                _same_bits(out, _run_gate_bwd(lib, cd, M, d, alpha, adaptive, extra, True)[1], log.tag)
    log.done()


@pytest.mark.parametrize("use_scratch", SCRATCH)
@pytest.mark.parametrize("cd", CDS)
def test_gate_saturated(lib, cd, use_scratch):
    """gate weights scaled until alpha is one-hot in every row: outputs finite, the logit gradient vanishes (dw / db keep their start value to rounding)"""
    M = 2049
    d, op = _gate_operands(cd, M, scale=1e6)
    out, alpha = _run_gate_fwd(lib, cd, M, d, 1)
    ref = R.gate_fwd_ref(op["xa"], op["xg"], op["xb"], op["w"], op["bias"], 1)
    log = Log(f"gate saturated {cd} scratch={use_scratch}")
    log.f32("alpha", _back(alpha[:, :3]), ref["alpha"], R.BAR32["gate_fwd"])
    log.stored("out", _back(out), ref["out"], cd, R.BAR32["gate_fwd"])
    assert float(ref["alpha"].max(1)[0].min()) > 1 - 1e-9, "the reference's alpha is not one-hot: the case does not saturate"
    rc, got = _run_gate_bwd(lib, cd, M, d, alpha, 1, True, use_scratch)
    assert rc == 0
    for n, t in got.items():
        assert bool(torch.isfinite(t).all()), n
    g = op["g"] + op["g1"] + op["g2"]
    rb = R.gate_bwd_ref(g, op["xa"], op["xg"], op["xb"], op["w"], _back(alpha[:, :3]), 1)
    for n in ("ga", "gg", "gb"):
        log.stored(n, got[n].double(), rb[n], cd, R.BAR32["gate_bwd"])
    unsat = float(R.gate_bwd_ref(g, op["xa"], op["xg"], op["xb"], op["w"], torch.full((M, 3), 1 / 3, dtype=torch.float64), 1)["dw"].abs().max())
    for n in ("dw", "db"):
        e = float((got[n].double() - 1 - rb[n]).abs().max())
        log.lines.append(f"{n} |got - ref| {e:.2e}, |ref| {float(rb[n].abs().max()):.2e} (unsaturated dw {unsat:.2e})")
        log.ok &= e <= R.BAR32["gate_bwd"] * unsat + _adds("gate", M, use_scratch) * 2.0 ** -23      # (each addition into the buffer holding 1 rounds at 2^-24 (1 + |dw|), |dw| < 1 here)
    log.done()
    if use_scratch:
        _same_bits(got, _run_gate_bwd(lib, cd, M, d, alpha, 1, True, True)[1], log.tag)


# ================================================================================================ head, rep
def _head_operands(cd, M):
    i = R.head_inputs(M)
    d = dict(rep=_dev(i["rep"], DT[cd][1]), w=_dev(i["w"]), bias=_dev(i["bias"]), dy=_dev(i["dy"]), drep=_dev(i["drep"]))
    op = {n: _back(t) for n, t in d.items()}
    assert float(op["rep"].abs().max()) == 1.0 and int((op["rep"].abs() == 1).sum()) >= (2 if M == 1 else 4)
    return d, op


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("M", R.HEAD_FWD_M)
def test_head_fwd(lib, cd, M):
    d, op = _head_operands(cd, M)
    out = _new((M, 3))
    _ok(lib.kasf_op_head_fwd(DT[cd][0], ptr(d["rep"]), ptr(d["w"]), ptr(d["bias"]), ptr(out), M, stream()), lib)
    log = Log(f"head_fwd {cd} M={M}")
    log.f32("out", _back(out), R.head_fwd_ref(op["rep"], op["w"], op["bias"]), R.BAR32["head_fwd"])
    log.done()


def _run_head_bwd(lib, cd, M, d, use_scratch, short=0):
    dpre, dw, db = _new((M, 512), DT[cd][1]), _new((3, 512), fill=1.0), _new(3, fill=1.0)
    sc, scn = _scratch(lib, 3, M, use_scratch, short)
    rc = lib.kasf_op_head_bwd(DT[cd][0], ptr(d["dy"]), ptr(d["rep"]), ptr(d["w"]), ptr(dpre), ptr(dw), ptr(db), M, ptr(sc), scn, stream())
    torch.cuda.synchronize()
    return rc, dict(dpre=dpre.cpu(), dw=dw.cpu(), db=db.cpu())


def _check_head_bwd(log, cd, out, op, adds):
    bar = R.BAR32["head_bwd"]
    ref = R.head_bwd_ref(op["dy"], op["rep"], op["w"])
    log.stored("dpre", out["dpre"].double(), ref["dpre"], cd, bar)
    log.f32("dw", out["dw"].double() - 1, ref["dw"], bar, adds=adds)
    log.f32("db", out["db"].double() - 1, ref["db"], bar, adds=adds)
    assert bool((out["dpre"][op["rep"].abs() == 1] == 0).all()), "dpre must be exactly 0 where rep is exactly +-1"


@pytest.mark.parametrize("use_scratch", SCRATCH)
@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("M", R.HEAD_BWD_M)
def test_head_bwd(lib, cd, M, use_scratch):
    d, op = _head_operands(cd, M)
    rc, out = _run_head_bwd(lib, cd, M, d, use_scratch)
    assert rc == 0, (rc, lib.kasf_last_error())
    log = Log(f"head_bwd {cd} M={M} scratch={use_scratch}")
    _check_head_bwd(log, cd, out, op, _adds("head", M, use_scratch))
    log.done()
    if use_scratch:
        _same_bits(out, _run_head_bwd(lib, cd, M, d, True)[1], log.tag)


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("M", R.REP_BWD_M)
def test_rep_bwd(lib, cd, M):
    d, op = _head_operands(cd, M)
    dpre = _new((M, 512), DT[cd][1])
    _ok(lib.kasf_op_rep_bwd(DT[cd][0], ptr(d["drep"]), ptr(d["rep"]), ptr(dpre), M, stream()), lib)
    log = Log(f"rep_bwd {cd} M={M}")
    log.stored("dpre", _back(dpre), R.rep_bwd_ref(op["drep"], op["rep"]), cd, R.BAR32["rep_bwd"])
    assert bool((dpre.cpu()[op["rep"].abs() == 1] == 0).all()), "dpre must be exactly 0 where rep is exactly +-1"
    log.done()


# ================================================================================================ layer-scale finish, add
@pytest.mark.parametrize("N,K", R.FINALIZE_NK)
def test_finalize_ls(lib, N, K):
    i = R.finalize_inputs(N, K)
    d = {n: _dev(t) for n, t in i.items()}
    dls = _new(N, fill=1.0)
    _ok(lib.kasf_op_finalize_ls(ptr(d["dw"]), ptr(d["w"]), ptr(d["bias"]), ptr(d["ls"]), ptr(d["db"]), ptr(dls), N, K, stream()), lib)
    ref = R.finalize_ref(*(i[n].double() for n in ("dw", "w", "bias", "ls", "db")))
    log, bar = Log(f"finalize_ls N={N} K={K}"), R.BAR32["finalize_ls"]
    log.f32("dw (scaled in place)", _back(d["dw"]), ref["dw"], bar)
    log.f32("db (scaled in place)", _back(d["db"]), ref["db"], bar)
    log.f32("dls", _back(dls) - 1, ref["dls"], bar, adds=1)
    for n in ("w", "bias", "ls"):
        assert torch.equal(d[n].cpu(), i[n]), f"{n} is an input"
    log.done()


@pytest.mark.parametrize("cd", CDS)
@pytest.mark.parametrize("n", R.ADD_N)
def test_add(lib, cd, n):
    code, dt = DT[cd]
    a, b, c, e = (_dev(t, dt) for t in R.add_inputs(n))
    A, B, Cc, E = (_back(t) for t in (a, b, c, e))
    log, bar = Log(f"add {cd} n={n}"), R.BAR32["add"]
    dst = _new(n, dt)
    _ok(lib.kasf_op_add(code, ptr(dst), ptr(a), ptr(b), None, n, stream()), lib)
    log.stored("a + b", _back(dst), A + B, cd, bar)
    dst = _new(n, dt)
    _ok(lib.kasf_op_add(code, ptr(dst), ptr(a), ptr(b), ptr(c), n, stream()), lib)
    log.stored("a + b + c", _back(dst), A + B + Cc, cd, bar)
    dst = e.clone()
    _KEEP.append(dst)
    _ok(lib.kasf_op_add(code, ptr(dst), ptr(a), None, None, n, stream()), lib)
    log.stored("dst += a", _back(dst), E + A, cd, bar)
    for t, want in ((a, A), (b, B), (c, Cc)):
        assert torch.equal(_back(t), want)
    log.done()


# ================================================================================================ scratch too small: error 6, and the atomics the launch fell back to
@pytest.mark.parametrize("cd", CDS)
def test_scratch_too_small_is_error_6(lib, models, cd):
    """One row short of what each op asks for: KasfColSink::take refuses, the launch runs on the fp32 atomics (gate_bwd: with its grid narrowed to the atomics' 256
    workgroups AFTER the refusal) and the entry reports 6 -- with complete, correct gradients."""
    log = Log(f"scratch too small {cd}")
    rc, out, ops = _run_embed(lib, cd, 129, True, True, short=64)
    assert rc == 6 and b"scratch" in lib.kasf_last_error(), (rc, lib.kasf_last_error())
    _check_embed(log, out, ops, True, _adds("embed", 129, False))
    rc, grads = _run_refusion(lib, models, 257, True, short=64)
    assert rc == 6
    _check_refusion(log, models, 257, grads, _adds("refusion", 257, False))
    M = 12291
    d, op = _gate_operands(cd, M)
    _, alpha = _run_gate_fwd(lib, cd, M, d, 1)
    rc, out = _run_gate_bwd(lib, cd, M, d, alpha, 1, True, True, short=64)
    assert rc == 6
    _check_gate_bwd(log, cd, out, op, alpha, 1, True, _adds("gate", M, False))
    d, op = _head_operands(cd, 4099)
    rc, out = _run_head_bwd(lib, cd, 4099, d, True, short=64)
    assert rc == 6
    _check_head_bwd(log, cd, out, op, _adds("head", 4099, False))
    # and a call with enough scratch afterwards is clean again
    rc, out, ops = _run_embed(lib, cd, 129, True, False)
    assert rc == 0
    log.done()
