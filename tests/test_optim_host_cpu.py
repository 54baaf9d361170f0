"""csrc/k_optim.hip without a GPU: the kernels' own source compiled for the host with g++ (-ffp-contract=off) behind the lockstep emulation of their workgroups
(tests/host_emul/) and held, bit for bit, to a numpy fp32 restatement of k_adamw's statements over a layout of odd segments (tests/optim_ref.py): sizes 1 to
8,193, begins of every residue mod 4, gaps, touching neighbours, two classes.  The k_adamw text of csrc/k_misc.hip is cut out as it is and compiled beside it for
the comparison with the one-range update.  What only the device can show (its sqrtf and divide, the real shuffles) stays with tests/test_gpu_optim.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kasportsformer_amd import _lib
from kasportsformer_amd.optim import CHUNK_DTYPE, plan_chunks
from tests import optim_ref as R
from tests.host_emul import CSRC, build, vp
from tests.optim_ref import F32, Guarded, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_CAP = 2048


def adamw_text():
    """ew_grid, k_adamw and its launcher as csrc/k_misc.hip has them."""
    src = open(os.path.join(CSRC, "k_misc.hip")).read()
    grid = re.search(r"^inline unsigned ew_grid\(.*?^}\n", src, re.S | re.M).group(0)
    kernel = re.search(r"^// torch\.optim\.AdamW semantics.*?^}\n", src, re.S | re.M).group(0)
    launcher = re.search(r"^void kasf_launch_adamw\(.*?^}\n", src, re.S | re.M).group(0)
    assert "void k_adamw(" in kernel and "k_adamw" in launcher
    return grid + kernel + launcher


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build(tmp_path_factory, "optim_host", "emul_optim.cpp", copy=("k_optim.hip",),
                 generate={"k_adamw.inc": adamw_text(), "kasf.h": open(os.path.join(ROOT, "include", "kasf.h")).read()})


def class_array(classes):
    arr = (_lib.KasfAdamwClass * len(classes))()
    for k, (lr, b1, b2, eps, wd, step) in enumerate(classes):
        bc1, bc2 = R.bias_corrections(b1, b2, step)
        arr[k] = _lib.KasfAdamwClass(lr, b1, b2, eps, wd, float(bc1), float(bc2), step)
    return arr


def table(segments=R.SEGMENTS):
    t = plan_chunks(*zip(*segments))
    assert t.dtype == CHUNK_DTYPE and t.itemsize == 16
    return t


def run_update(lib, arrs, segments=R.SEGMENTS, classes=R.CLASSES, grad_scale=1.0, clip=None, tbl=None, n_chunks=None):
    """One emulated kasf_launch_adamw_segments over guarded copies of p, g, m, v -> (launches, [Guarded x 4])."""
    guards = [Guarded(a) for a in arrs]
    tbl = table(segments) if tbl is None else tbl
    cl = None if clip is None else np.asarray(clip, F32)
    n = lib.emul_adamw_segments(*(vp(q.data) for q in guards), vp(tbl), C.c_int64(len(tbl) if n_chunks is None else n_chunks), class_array(classes),
                                len(classes), C.c_float(grad_scale), None if cl is None else vp(cl), GRID_CAP)
    return n, guards


def run_norm(lib, g, tbl, grad_scale=1.0, max_norm=1.0, grid_cap=GRID_CAP):
    gg, out2, partial = Guarded(g), Guarded(np.full(2, -7.0, F32)), np.full(len(tbl) + 1, -3.0)
    n = lib.emul_grad_norm(vp(gg.data), vp(tbl), C.c_int64(len(tbl)), vp(partial), C.c_float(grad_scale), C.c_float(max_norm), vp(out2.data), grid_cap)
    assert gg.canaries_intact() and out2.canaries_intact() and partial[len(tbl)] == -3.0 and np.array_equal(bits(gg.data), bits(g))
    return n, out2.data.copy(), partial[:len(tbl)].copy()


def test_the_layout_is_the_one_the_issue_names():
    sizes = sorted(c for _, c, _ in R.SEGMENTS)
    assert sizes == [1, 2, 3, 4, 5, 16, 17, 4095, 4097, 8193] and R.N_FLAT == 20000
    assert {b % 4 for b, _, _ in R.SEGMENTS} == {0, 1, 2, 3}
    ends = {b + c for b, c, _ in R.SEGMENTS}
    gaps = sorted(b - max(e for e in ends | {0} if e <= b) for b, _, _ in R.SEGMENTS)
    assert gaps.count(0) == 2 and set(gaps) - {0} <= set(range(1, 8)) and len(set(gaps)) >= 6
    t = table()
    big = t[(t["begin"] >= 8271) & (t["begin"] < 8271 + 8193)]
    assert len(big) >= 3, "the largest segment crosses at least two chunk boundaries"
    a, b = R.CLASSES
    assert a[0] != b[0] and a[4] != b[4] and a[5] != b[5]


@pytest.mark.parametrize("grad_scale", [1.0, 0.37])
def test_segmented_update_has_the_bits_of_the_restated_statements(emul, grad_scale):
    arrs = R.payloads(1)
    n, guards = run_update(emul, arrs, grad_scale=grad_scale)
    assert n == 1, "one launch"
    want = R.expected(arrs, F32(grad_scale))
    mask = R.listed_mask()
    for name, q, w, before in zip("pgmv", guards, want, arrs):
        assert q.canaries_intact(), name
        assert np.array_equal(bits(q.data)[~mask], bits(before)[~mask]), f"{name}: an element outside the listed ones changed"
        assert np.array_equal(bits(q.data)[mask], bits(w)[mask]), f"{name}: listed elements differ from the restatement"
    assert not np.array_equal(bits(guards[0].data)[mask], bits(arrs[0])[mask])


def test_one_class_one_run_has_the_bits_of_k_adamw(emul):
    n_el = 4096
    arrs = [a[:n_el] for a in R.payloads(2)]
    cls = R.CLASSES[0]
    n, guards = run_update(emul, arrs, segments=[(0, n_el, 0)], classes=[cls], grad_scale=0.5)
    assert n == 1
    old = [Guarded(a) for a in arrs]
    bc1, bc2 = R.bias_corrections(cls[1], cls[2], cls[5])
    n_old = emul.emul_adamw(*(vp(q.data) for q in old), C.c_int64(n_el), *(C.c_float(x) for x in cls[:5]), C.c_float(bc1), C.c_float(bc2), C.c_float(0.5))
    assert n_old == 1
    for name, a, b, before in zip("pgmv", guards, old, arrs):
        assert a.canaries_intact() and b.canaries_intact()
        assert np.array_equal(bits(a.data), bits(b.data)), name
    assert not np.array_equal(bits(guards[0].data), bits(arrs[0]))


def test_norm_value_bits_and_grid_width(emul):
    arrs = R.payloads(3)
    g, mask, tbl = arrs[1], R.listed_mask(), table()
    for gs in (1.0, 0.25):
        n, out2, partial = run_norm(emul, g, tbl, grad_scale=gs, max_norm=1.0)
        assert n == 2, "the per-chunk pass and the finish"
        want = R.norm_ref(g, mask, gs)
        rel = abs(float(out2[0]) - want) / want
        print(f"grad_scale {gs}: norm {out2[0]!r} against {want!r}: relative error {rel:.3e} (bound {2.0 ** -22:.3e})")
        assert rel <= 2.0 ** -22
        assert out2[1] == min(F32(1.0), F32(1.0) / (out2[0] + F32(1e-6)))
        _, again, partial2 = run_norm(emul, g, tbl, grad_scale=gs, max_norm=1.0)
        assert np.array_equal(bits(again), bits(out2)) and np.array_equal(partial.view(np.uint64), partial2.view(np.uint64))
        for cap in (1, 3):
            _, narrow, partial3 = run_norm(emul, g, tbl, grad_scale=gs, max_norm=1.0, grid_cap=cap)
            assert np.array_equal(bits(narrow), bits(out2)) and np.array_equal(partial.view(np.uint64), partial3.view(np.uint64)), cap
    # each chunk's double against numpy's over the same elements: the order differs, the value to 1e-12
    for c, got in zip(tbl, partial):
        ref = (g[c["begin"]:c["begin"] + c["count"]].astype(np.float64) ** 2).sum()
        assert abs(got - ref) <= 1e-12 * max(ref, 1e-300)


def test_norm_special_values(emul):
    g, tbl = R.payloads(4)[1], table()
    _, out2, _ = run_norm(emul, g, tbl, max_norm=float("inf"))
    assert np.isfinite(out2[0]) and bits(out2[1:])[0] == bits(F32(1.0)), "max_norm = inf measures: the coefficient is 1.0f exactly"
    gi = g.copy(); gi[4171] = np.inf
    _, out2, _ = run_norm(emul, gi, tbl, max_norm=1.0)
    assert np.isposinf(out2[0]) and out2[1] == 0.0
    gn = g.copy(); gn[30] = np.nan
    _, out2, _ = run_norm(emul, gn, tbl, max_norm=1.0)
    assert np.isnan(out2[0]) and np.isnan(out2[1])
    go = g.copy(); go[0] = np.inf; go[6] = np.nan        # elements outside every chunk take no part
    _, out2, _ = run_norm(emul, go, tbl, max_norm=1.0)
    assert np.isfinite(out2).all()


def test_a_clip_coefficient_of_one_changes_no_bit(emul):
    arrs = R.payloads(5)
    _, plain = run_update(emul, arrs, grad_scale=0.37)
    _, clipped = run_update(emul, arrs, grad_scale=0.37, clip=[123.0, 1.0])
    _, half = run_update(emul, arrs, grad_scale=0.37, clip=[123.0, 0.5])
    for a, b in zip(plain, clipped):
        assert np.array_equal(bits(a.data), bits(b.data))
    want = R.expected(arrs, F32(0.37) * F32(0.5))
    mask = R.listed_mask()
    for q, w in zip(half, want):
        assert q.canaries_intact() and np.array_equal(bits(q.data)[mask], bits(w)[mask])


def test_no_chunks_touch_nothing(emul):
    arrs = R.payloads(6)
    n, guards = run_update(emul, arrs, n_chunks=0)
    assert n == 0
    for q, before in zip(guards, arrs):
        assert q.canaries_intact() and np.array_equal(bits(q.data), bits(before))
    out2, partial = np.full(2, -7.0, F32), np.full(4, -3.0)
    assert emul.emul_grad_norm(vp(arrs[1]), vp(table()), C.c_int64(0), vp(partial), C.c_float(1.0), C.c_float(1.0), vp(out2), GRID_CAP) == 0
    assert (out2 == -7.0).all() and (partial == -3.0).all()
