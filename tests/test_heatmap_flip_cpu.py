"""Host side of the flip-tested heatmap decode (kasportsformer_amd.heatmaps_to_keypoints(flipped=...), push_heatmaps(flipped=...),
kasf_heatmap_flip_keypoints): the numpy restatement the GPU tests hold the kernel to (tests/test_gpu_heatmap_flip.py imports it from here), built from the index
formula of include/kasf.h plus tests/test_heatmap_cpu.py's heatmap_decode_np, and tied to the fixture the reference's own flip_back and get_final_preds wrote
(tests/golden/make_heatmap_flip_golden.py); the refusals of the entry point and of the Python surface."""
import contextlib
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_heatmap_cpu import F32, GOLDEN, GROUPS, heatmap_decode_np, same_bits, ulp_distance

COCO_PAIRS = ((1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16))
SIZES = {"a": (96, 72), "b": (64, 48)}


def fixture():
    return np.load(os.path.join(GOLDEN, "heatmap_flip.npz"), allow_pickle=False)


def partner_np(pairs=COCO_PAIRS):
    t = np.arange(17)
    for a, b in pairs:
        t[a], t[b] = b, a
    return t


def src_x_np(W, shift):
    """Column of the flipped map that column x of the merged map takes (include/kasf.h): shift ? min(W - x, W - 1) : W - 1 - x."""
    x = np.arange(W)
    return np.minimum(W - x, W - 1) if shift else W - 1 - x


def widen(a):
    a = a.float().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a if a.dtype == F32 else a.astype(F32)


def merge_np(hm, hmf, *, shift=True, partner=None):
    """merged[p][j][y][x] = (hm[p][j][y][x] + hmf[p][partner[j]][y][src_x(x)]) * 0.5f on the float32 values (16-bit input widened exactly): one fp32 add, one
    fp32 multiply -> float32 [n,17,H,W]."""
    a, b = widen(hm), widen(hmf)
    partner = partner_np() if partner is None else np.asarray(partner)
    with np.errstate(invalid="ignore"):
        merged = (a + b[:, partner][..., src_x_np(a.shape[-1], shift)]) * F32(0.5)
    assert merged.dtype == F32
    return merged


def heatmap_flip_decode_np(hm, hmf, center=None, scale=None, *, shift=True, partner=None, refine=True, boxes=None, aspect=None, parts=False):
    """The flip test restated: merge_np, then heatmap_decode_np of the merged maps -> [n,17,3] float32; with parts=True
    (out, argmax positions, refined heatmap coordinates, merged)."""
    merged = merge_np(hm, hmf, shift=shift, partner=partner)
    got = heatmap_decode_np(merged, center, scale, boxes=boxes, aspect=aspect, refine=refine, parts=parts)
    return got + (merged,) if parts else got


def flip_back_and_shift_np(hmf, pairs, shift):
    """HRNet's procedure on a copy, as the reference writes it: flip_back (transforms.py:15-30: reverse the columns, swap each pair's maps), then
    output_flipped[:, :, :, 1:] = output_flipped.clone()[:, :, :, 0:-1]."""
    out = np.array(hmf[:, :, :, ::-1])
    for a, b in pairs:
        tmp = out[:, a].copy()
        out[:, a] = out[:, b]
        out[:, b] = tmp
    if shift:
        out[:, :, :, 1:] = out.copy()[:, :, :, 0:-1]
    return out


def test_fixture_loads_without_pickles_and_is_small():
    path = os.path.join(GOLDEN, "heatmap_flip.npz")
    assert os.path.getsize(path) < 400 * 1024
    fx = fixture()
    for g in GROUPS:
        H, W = SIZES[g]
        hm, hmf = fx[g + "_hm"], fx[g + "_hmf"]
        P = hm.shape[0]
        assert hm.dtype == hmf.dtype == np.float16 and hm.shape == hmf.shape == (P, 17, H, W) and P >= 4
        assert fx[g + "_merged"].dtype == F32 and fx[g + "_merged"].shape == hm.shape
        assert fx[g + "_center"].shape == fx[g + "_scale"].shape == (P, 2)
        assert fx[g + "_maxvals"].shape == (P, 17, 1) and fx[g + "_maxpos"].shape == (P, 17, 2)
        for r in (0, 1):
            assert fx[f"{g}_preds_r{r}"].shape == fx[f"{g}_coords_r{r}"].shape == (P, 17, 2) and fx[f"{g}_preds_r{r}"].dtype == F32


def test_restatement_is_the_reference_on_the_fixture():
    """merged and maxvals bit for bit (the reference's flip_back, slice-assignment shift and float32 average against the index formula), argmax positions
    and refined coordinates bit for bit, image-space preds within the 1 fp32 ulp of tests/test_heatmap_cpu.py's fixture test (the shim's float64 solve against
    the closed form), and no more coordinates off than the generator counted."""
    fx = fixture()
    neq, worst = 0, 0
    for g in GROUPS:
        for r in (0, 1):
            out, pos, coords, merged = heatmap_flip_decode_np(fx[g + "_hm"], fx[g + "_hmf"], fx[g + "_center"], fx[g + "_scale"], refine=bool(r), parts=True)
            assert same_bits(merged, fx[g + "_merged"])
            assert same_bits(out[..., 2], fx[g + "_maxvals"][..., 0])
            assert same_bits(pos, fx[g + "_maxpos"]) and same_bits(coords, fx[f"{g}_coords_r{r}"])
            d = ulp_distance(out[..., :2], fx[f"{g}_preds_r{r}"])
            neq, worst = neq + int((d != 0).sum()), max(worst, int(d.max()))
    print(f"restatement vs reference: {neq} coordinates not bit-equal (recorded {int(fx['neq_count'])}), largest distance {worst} ulp")
    assert worst <= 1
    assert neq <= int(fx["neq_count"]) and int(fx["max_ulp"]) <= 1


@pytest.mark.parametrize("g", GROUPS)
def test_the_merge_decided_every_hand_made_case(g):
    """The last person of each group, maps as make_heatmap_flip_golden.merge_person lays them out: positions, scores and refinement steps of the merged maps,
    and what each operand alone would have said."""
    fx = fixture()
    H, W = SIZES[g]
    hm, hmf = fx[g + "_hm"][-1:].astype(F32), fx[g + "_hmf"][-1:].astype(F32)
    pos, val = fx[g + "_maxpos"][-1], fx[g + "_maxvals"][-1, :, 0]
    step = fx[g + "_coords_r1"][-1] - pos
    merged = fx[g + "_merged"][-1]
    zeros = np.zeros((1, 2), F32)
    direct = heatmap_decode_np(hm, zeros, zeros + 1, parts=True)[1][0]               # the argmax positions of the direct operand alone
    back = flip_back_and_shift_np(hmf, COCO_PAIRS, True)
    flipped = heatmap_decode_np(back, zeros, zeros + 1, parts=True)[1][0]            # ... and of the flipped operand, mirrored back and shifted
    at = lambda j: (int(pos[j, 0]), int(pos[j, 1]))
    # 0 (unpaired): the maximum exists only in the flipped operand
    assert at(0) == (W - 30, 9) and val[0] == 0.5 and tuple(flipped[0]) == at(0) and tuple(direct[0]) != at(0) and hm[0, 0].max() == 0.25
    # 1, 2: two equal merged maxima; the first in row-major order comes from the direct operand (1) and from the flipped one (2)
    for j, first in ((1, direct), (2, flipped)):
        assert (merged[j] == merged[j].max()).sum() == 2 and val[j] == 0.25
        assert tuple(first[j]) == at(j) and tuple((flipped if first is direct else direct)[j]) != at(j)
        assert at(j)[1] < max(direct[j, 1], flipped[j, 1]), "the other maximum lies in a later row"
    # 3-6: peaks at x = 0, 1, W - 2, W - 1.  3: the flipped map's last column lands on columns 0 AND 1 (the shift's edge): a tie, column 0 first
    assert at(3) == (0, H // 2) and merged[3, H // 2, 0] == merged[3, H // 2, 1] == val[3] == 0.5
    assert at(4) == (1, H // 2) and val[4] == 0.75 and at(5) == (W - 2, H // 2) and at(6) == (W - 1, H // 2)
    assert tuple(flipped[5]) == at(5) and tuple(flipped[6]) == at(6) and direct[5].sum() == 0 and direct[6].sum() == 0
    assert hmf[0, 5, H // 2, 0] == 2.0 and val[6] == 0.5, "column 0 of a flipped map is shifted out: its 2.0 reaches no merged value"
    for j in (3, 4, 6):
        assert not step[j].any(), "x = 0, 1, W - 1 are outside the strict bounds"
    assert tuple(step[5]) == (0.25, 0.25), "x = W - 2 is refined, from merged neighbours that come from the flipped operand"
    # 7: equal merged neighbours in x although each operand's differ: sign(0) = 0
    x, y = at(7)
    assert merged[7, y, x - 1] == merged[7, y, x + 1] and hm[0, 7, y, x - 1] != hm[0, 7, y, x + 1] and tuple(step[7]) == (0, 0.25)
    # 8, 9: merged maxima that are zero and negative although one operand has a positive peak: (0, 0), unrefined
    assert val[8] == 0 and val[9] == -0.25 and hmf[0, 7].max() > 0 and hm[0, 9].max() > 0
    assert not pos[[8, 9]].any() and not step[[8, 9]].any()
    # 10: both operands peak, one column apart; the merged maximum is where neither operand alone has its own
    assert at(10) == (31, H - 14) and tuple(direct[10]) == (30, H - 14) and val[10] == 0.875
    # 11, 12: a pair whose operands disagree on the side: the larger merged value wins, from the flipped operand (11) and from the direct one (12)
    assert at(11) == tuple(flipped[11]) != tuple(direct[11]) and val[11] == 0.5 and abs(int(direct[11, 0]) - at(11)[0]) > W // 3
    assert at(12) == tuple(direct[12]) != tuple(flipped[12]) and val[12] == 0.5
    # 13, 14: the first and the last refined column, one from each operand
    assert at(13) == (2, 2) and tuple(step[13]) == (0.25, -0.25) and at(14) == (W - 3, H - 3) and tuple(step[14]) == (-0.25, 0.25)
    assert tuple(direct[14]) == (0, 0) and tuple(flipped[14]) == at(14)
    # 15: both operands peak on the same merged pixel; 16: nothing anywhere
    assert at(15) == (35, H - 20) and val[15] == 0.625 and at(16) == (0, 0) and val[16] == 0
    assert np.array_equal(fx[g + "_coords_r0"], fx[g + "_maxpos"])


@pytest.mark.parametrize("shift", [True, False])
def test_the_index_formula_is_flip_back_and_the_slice_assignment(shift):
    g = np.random.default_rng(7)
    for W in range(1, 10):
        hmf = g.normal(size=(2, 17, 3, W)).astype(F32)
        for pairs in (COCO_PAIRS, ((5, 6),), ()):
            want = flip_back_and_shift_np(hmf, pairs, shift)
            assert np.array_equal(hmf[:, partner_np(pairs)][..., src_x_np(W, shift)], want), (W, pairs)
            hm = g.normal(size=hmf.shape).astype(F32)
            assert same_bits(merge_np(hm, hmf, shift=shift, partner=partner_np(pairs)), (hm + want) * F32(0.5))
    assert src_x_np(1, True).tolist() == [0] and src_x_np(2, True).tolist() == [1, 1] and src_x_np(4, True).tolist() == [3, 3, 2, 1]


def test_sixteen_bit_operands_merge_as_their_upcasts_not_in_half():
    a, b = np.full((1, 17, 2, 2), 0.1, np.float16), np.full((1, 17, 2, 2), 2049.0, np.float16)
    merged = merge_np(a, b)
    assert same_bits(merged, merge_np(a.astype(F32), b.astype(F32)))
    assert not np.array_equal(merged, ((a + b) * np.float16(0.5)).astype(F32)), "half arithmetic rounds the sum; the rule does not"


def test_entry_point_refuses_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    assert "kasf_heatmap_flip_keypoints" in _lib.SIGNATURES and hasattr(lib, "kasf_heatmap_flip_keypoints")
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "kasf.h")).read()
    assert "int kasf_heatmap_flip_keypoints(const void* hm, const void* hm_flipped, int32_t dtype, int64_t n, int32_t H, int32_t W," in hdr
    assert "src_x(x)           = shift ? min(W - x, W - 1) : W - 1 - x" in hdr
    assert _lib.ABI_VERSION == lib.kasf_version() == 12
    hm, hmf, geom = np.full(17 * 15, 3, F32), np.full(17 * 15, 4, F32), np.full(4, 5, F32)
    out, tmp, mrg = np.full(51, 7, F32), np.full(51, 9, F32), np.full(17 * 15, 11, F32)
    p = [a.ctypes.data_as(C.c_void_p) for a in (hm, hmf, geom, out, tmp, mrg)]
    f = lib.kasf_heatmap_flip_keypoints

    def table(t):
        return None if t is None else np.asarray(t, np.int32).ctypes.data_as(C.c_void_p)

    def call(hm=p[0], hmf=p[1], dtype=0, n=1, H=5, W=3, partner=None, shift=1, geom=p[2], kind=0, aspect=1.0, refine=1, layout=0, out=p[3], tmp=p[4],
             merged=None):
        keep = None if partner is None else np.ascontiguousarray(partner, dtype=np.int32)
        return f(hm, hmf, dtype, n, H, W, None if keep is None else keep.ctypes.data_as(C.c_void_p), shift, geom, kind, aspect, refine, layout, out, tmp,
                 merged, None)

    assert call(n=0) == 0 and call(None, None, n=0, geom=None, out=None, tmp=None) == 0          # nothing to do
    assert call(n=0, partner=partner_np()) == 0 and call(n=0, partner=np.arange(17)) == 0
    swapped = np.arange(17)
    swapped[[0, 16]] = 16, 0
    assert call(n=0, partner=swapped) == 0
    cycle = np.arange(17)
    cycle[[1, 2, 3]] = 2, 3, 1                                  # a permutation that is no involution
    twice = partner_np()
    twice[3] = 1                                                # 1 <-> 2 and 3 -> 1
    high, low = partner_np(), partner_np()
    high[0], low[16] = 17, -1
    refused = [dict(n=-1), dict(H=0), dict(W=0), dict(H=-5), dict(H=4097, W=4096), dict(H=1 << 30, W=1 << 30), dict(dtype=3), dict(dtype=-1),
               dict(kind=2), dict(kind=-1), dict(layout=2), dict(layout=-1), dict(kind=1, aspect=0.0), dict(kind=1, aspect=-0.5),
               dict(kind=1, aspect=float("nan")), dict(hm=None), dict(hmf=None), dict(geom=None), dict(out=None), dict(layout=1, tmp=None),
               dict(partner=cycle), dict(partner=twice), dict(partner=high), dict(partner=low), dict(partner=np.zeros(17)), dict(n=0, partner=cycle),
               dict(merged=p[0]), dict(merged=p[1])]
    for kw in refused:
        assert call(**kw) == 2, kw
        assert lib.kasf_last_error(), kw
    assert (hm == 3).all() and (hmf == 4).all() and (geom == 5).all() and (out == 7).all() and (tmp == 9).all() and (mrg == 11).all(), \
        "a refused call touches no buffer"


def test_partner_table_validation():
    from kasportsformer_amd import heatmap
    who = "t"
    assert heatmap.partner_table(None, who).tolist() == partner_np().tolist() and heatmap.COCO_PAIRS == COCO_PAIRS
    assert heatmap.partner_table([], who).tolist() == list(range(17))
    assert heatmap.partner_table([(5, 6)], who).tolist() == partner_np(((5, 6),)).tolist()
    assert heatmap.partner_table(np.array([[0, 16], [3, 2]]), who).tolist() == partner_np(((0, 16), (3, 2))).tolist()
    for exc, pairs in ((ValueError, [(1, 2), (2, 3)]), (ValueError, [(1, 2), (1, 2)]), (ValueError, [(4, 4)]), (ValueError, [(0, 17)]), (ValueError, [(-1, 3)]),
                       (ValueError, [(1, 2, 3)]), (ValueError, [(1,)]), (ValueError, [5]), (TypeError, [(1.0, 2.0)]), (TypeError, [("a", "b")]),
                       (TypeError, [(True, 2)]), (TypeError, 5), (TypeError, "12")):
        with pytest.raises(exc):
            heatmap.partner_table(pairs, who)


@pytest.fixture
def no_launch(monkeypatch):
    """The loader refuses: whatever reaches the library fails the test."""
    from kasportsformer_amd import _lib

    def load():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", load)


def flip_refusals(call, hm, c, s):
    """Every new ValueError / TypeError of an entry point `call(hm, c, s, **kw)`."""
    f = hm.copy()
    return ((ValueError, lambda: call(hm, c, s, shift=False)),
            (ValueError, lambda: call(hm, c, s, pairs=[(1, 2)])),
            (ValueError, lambda: call(hm, c, s, pairs=[])),
            (ValueError, lambda: call(hm, c, s, flipped=f[:, :, :4])),
            (ValueError, lambda: call(hm, c, s, flipped=f[:1])),
            (ValueError, lambda: call(hm, c, s, flipped=f.astype(np.float16))),
            (TypeError, lambda: call(hm, c, s, flipped=f.astype(np.float64))),
            (TypeError, lambda: call(hm, c, s, flipped=f.tolist())),
            (TypeError, lambda: call(hm, c, s, flipped=f, shift=1)),
            (TypeError, lambda: call(hm, c, s, flipped=f, shift=None)),
            (ValueError, lambda: call(hm, c, s, flipped=f, pairs=[(1, 2), (2, 3)])),
            (ValueError, lambda: call(hm, c, s, flipped=f, pairs=[(0, 17)])),
            (ValueError, lambda: call(hm, c, s, flipped=f, pairs=[(1, 2, 3)])),
            (TypeError, lambda: call(hm, c, s, flipped=f, pairs=[(1.5, 2)])),
            (TypeError, lambda: call(hm, c, s, flipped=f, pairs=7)))


def test_heatmaps_to_keypoints_refuses_before_any_launch(no_launch):
    import kasportsformer_amd as K
    assert "flip test" in K.__doc__
    hm = np.zeros((2, 17, 5, 3), F32)
    c, s = np.zeros((2, 2), F32), np.ones((2, 2), F32)
    h = K.heatmaps_to_keypoints
    for exc, call in flip_refusals(h, hm, c, s) + (
            (ValueError, lambda: h(hm, c, s, merged=True)),
            (ValueError, lambda: h(hm, c, s, merged=torch.zeros(2, 17, 5, 3))),
            (TypeError, lambda: h(hm, c, s, flipped=hm, merged=np.zeros((2, 17, 5, 3), F32))),
            (TypeError, lambda: h(hm, c, s, flipped=hm, merged=1)),
            (TypeError, lambda: h(hm, c, s, flipped=hm, merged=torch.zeros((2, 17, 5, 3), dtype=torch.float16))),
            (RuntimeError, lambda: h(hm, c, s, flipped=hm, merged=torch.zeros(2, 17, 5, 3))),            # float32, but on the host
            (RuntimeError, lambda: h(hm, c, s, flipped=hm, device="cpu"))):
        with pytest.raises(exc):
            call()
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            h(hm, c, s, flipped=hm)
        with pytest.raises(RuntimeError, match="no CPU path"):
            h(hm, c, s, flipped=hm, shift=False, pairs=[(5, 6)], merged=True, layout="h36m")
    assert not hm.any() and not c.any()


def bare(cls, **attrs):
    """An instance without __init__ (which needs a GPU): only what push_heatmaps reads before it decodes."""
    obj = object.__new__(cls)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_push_heatmaps_refuse_before_any_launch(no_launch):
    import kasportsformer_amd as K
    hm = np.zeros((2, 17, 5, 3), F32)
    c, s = np.zeros((2, 2), F32), np.ones((2, 2), F32)
    stream = bare(K.StreamLifter, slots=2, _coco=False, device=torch.device("cuda", 0))
    tracked = bare(K.TrackedLifter, streams=1, R=2, _coco=False, device=torch.device("cuda", 0))
    for lifter in (stream, tracked):
        for exc, call in flip_refusals(lifter.push_heatmaps, hm, c, s):
            with pytest.raises(exc):
                call()
    for cls in (K.StreamLifter, K.TrackedLifter):
        params = inspect.signature(cls.push_heatmaps).parameters
        for name, default in (("flipped", None), ("shift", True), ("pairs", None)):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is default
    params = inspect.signature(K.heatmaps_to_keypoints).parameters
    for name, default in (("flipped", None), ("shift", True), ("pairs", None), ("merged", None)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default is default


class RecordingLib:
    """Stands in for the loaded library: records which entry was called with what, and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            if name == "kasf_heatmap_flip_keypoints":            # the partner table is host memory that lives for the call: copy it now
                args = args[:6] + (np.ctypeslib.as_array(C.cast(args[6], C.POINTER(C.c_int32)), (17,)).tolist(),) + args[7:]
            self.calls.append((name, args))
            return 0
        return entry


def test_without_flipped_the_old_entry_is_called_and_with_it_the_new_one(monkeypatch):
    from kasportsformer_amd import _args, _lib, heatmap
    lib = RecordingLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_args, "stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    hm, hmf = torch.zeros((2, 17, 5, 3)), torch.ones((2, 17, 5, 3))
    parts = (torch.zeros((2, 2)), torch.ones((2, 2)))
    out = heatmap.decode(hm, parts, _lib.GEOM_CENTER_SCALE, 1.0, True, False)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (2, 17, 3)
    (name, args), = lib.calls
    assert name == "kasf_heatmap_keypoints" and len(args) == 13 and args[:5] == (hm.data_ptr(), _lib.DTYPE_F32, 2, 5, 3)
    del lib.calls[:]
    flip = heatmap.check_flip_args(hm, hmf, False, [(5, 6)], "t")
    out, merged = heatmap.decode(hm, parts, _lib.GEOM_CENTER_SCALE, 1.0, False, False, flip, True)
    (name, args), = lib.calls
    assert name == "kasf_heatmap_flip_keypoints" and len(args) == 17
    assert args[:6] == (hm.data_ptr(), hmf.data_ptr(), _lib.DTYPE_F32, 2, 5, 3) and args[7] == 0 and args[11] == 0 and args[15] == merged.data_ptr()
    assert args[6] == partner_np(((5, 6),)).tolist()
    assert merged.dtype == torch.float32 and tuple(merged.shape) == (2, 17, 5, 3)
    del lib.calls[:]
    assert isinstance(heatmap.decode(hm, parts, _lib.GEOM_CENTER_SCALE, 1.0, True, False, heatmap.check_flip_args(hm, hmf, True, None, "t")), torch.Tensor)
    assert lib.calls[0][1][15] is None and lib.calls[0][1][7] == 1, "no merged output unless asked for"
    assert heatmap.check_flip_args(hm, None, True, None, "t") is None
    del lib.calls[:]
    for table in (np.arange(16), np.arange(18), np.arange(34).reshape(2, 17)):      # a table of the wrong length never reaches the library
        with pytest.raises(ValueError):
            heatmap.decode(hm, parts, _lib.GEOM_CENTER_SCALE, 1.0, True, False, (hmf, True, table))
    assert not lib.calls


def test_push_heatmaps_needs_a_gpu_as_before():
    import kasportsformer_amd as K
    m = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=27, compute_dtype="fp32")
    with pytest.raises(RuntimeError):
        K.StreamLifter(m, 1280, 720, slots=2)
    with pytest.raises(RuntimeError):
        K.TrackedLifter(m, 1280, 720)
