"""csrc/k_bones.hip without a GPU: the kernels' own source compiled for the host with g++ behind the lockstep emulation of a workgroup (tests/host_emul/) and
held to the numpy restatement of include/kasf.h's rule (tests/bones_ref.py) bit for bit: medians and counts, walked frames, len / cnt / owner after every tick,
row_slot, canaries around every array, inputs unchanged.  It shows the kernels' logic, their indexing and their fp32 operation order; what only the device can
show (its square root and divide, its atomics) stays with tests/test_gpu_bones.py."""
import ctypes as C

import numpy as np
import pytest

from tests import bones_ref as R
from tests import smooth_ref
from tests.host_emul import build, vp
from tests.tracked_ref import Cases, script

PAD = 64
B, S_T, T = 2, 4, 5


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build(tmp_path_factory, "bones_host", "emul_bones.cpp")


class Guarded:
    """An array with PAD canary elements on either side."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.canary = np.frombuffer(bytes([0x5A]) * np.dtype(dtype).itemsize, dtype)[0]
        self.buf = np.full(n + 2 * PAD, self.canary, dtype)
        self.a = self.buf[PAD:PAD + n].reshape(shape)
        self.a[...] = fill

    def intact(self):
        raw, w = self.buf.view(np.uint8), PAD * self.buf.itemsize
        c = np.frombuffer(self.canary.tobytes(), np.uint8)
        return bool((raw[:w].reshape(PAD, -1) == c).all() and (raw[len(raw) - w:].reshape(PAD, -1) == c).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def where_differs(a, b):
    return np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4]


@pytest.mark.parametrize("with_counts", [True, False])
def test_select_finds_the_lower_median_of_any_bit_patterns(emul, with_counts):
    s, off = R.select_scratch()
    keep, P, N = s.copy(), len(off) - 1, s.shape[1]
    want_L, want_n = R.median_of_scratch_np(s, off)
    L, n = Guarded((P, 16), np.float32, 9.0), Guarded((P, 16), np.int32, -7)
    emul.emul_select(vp(s), vp(off), C.c_int64(N), P, vp(L.a), vp(n.a) if with_counts else None)
    assert same_bits(L.a, want_L), where_differs(L.a, want_L)
    assert np.array_equal(n.a, want_n if with_counts else np.full((P, 16), -7, np.int32))
    assert L.intact() and n.intact() and same_bits(s, keep)
    assert (want_n == 0).any() and (want_n[7] == 300).any() and (want_L[:, 3][want_n[:, 3] > 0] < np.float32(1.2e-38)).all()      # empty, one past a pass, denormal medians


def test_median_over_tracks_of_every_kind(emul):
    x, off = R.median_tracks()
    keep, P, N = x.copy(), len(off) - 1, len(x)
    want_L, want_n = R.median_np(x, off)
    scratch, L, n = Guarded((16, N), np.float32, 9.0), Guarded((P, 16), np.float32, 9.0), Guarded((P, 16), np.int32, -7)
    emul.emul_lengths(vp(x), C.c_int64(N), vp(scratch.a))
    emul.emul_select(vp(scratch.a), vp(off), C.c_int64(N), P, vp(L.a), vp(n.a))
    assert same_bits(L.a, want_L), where_differs(L.a, want_L)
    assert np.array_equal(n.a, want_n)
    assert scratch.intact() and L.intact() and n.intact() and same_bits(x, keep)
    lengths = np.diff(off)
    assert set(R.MEDIAN_LENGTHS) <= set(lengths.tolist()) and lengths[1] == 0 and lengths[0] > 0 and lengths[2] > 0      # an empty track between two others
    assert (want_n[-3] == 0).all() and (want_n[-2] == 0).all() and (want_n[-4] < lengths[-4]).all() and (want_n[-4] > 0).all()   # no usable frame; overflow; NaN frames
    assert want_n[-5][1] == 0 and 0 < want_n[-5][15] < lengths[-5]                                                        # zero-length bones
    # offsets outside [0, N] and descending ones are clamped, as k_one_euro_tracks clamps them
    odd = np.array([-5, 3, 2, N + 9], np.int64)
    L2, n2 = Guarded((3, 16), np.float32, 9.0), Guarded((3, 16), np.int32, -7)
    emul.emul_select(vp(scratch.a), vp(odd), C.c_int64(N), 3, vp(L2.a), vp(n2.a))
    w_L, w_n = R.median_np(x, np.array([0, 3, 3, N]))
    w_L[2], w_n[2] = R.median_np(x, np.array([2, N]))
    assert same_bits(L2.a, w_L) and np.array_equal(n2.a, w_n) and L2.intact() and n2.intact()


def apply_tables(L):
    """The per-track table as found, with one partner 0, and with bones (a pair among them) left alone."""
    one, none = L.copy(), L.copy()
    one[:, 3], one[1::2, 10] = 0, 0
    none[:, [1, 4, 7, 15]] = 0
    return {"medians": L, "one_partner_0": one, "L_0": none}


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("table", ["medians", "one_partner_0", "L_0"])
def test_apply_walks_every_frame_with_its_tracks_table(emul, table, symmetric):
    x, off = R.median_tracks()
    keep, P, N = x.copy(), len(off) - 1, len(x)
    L = apply_tables(R.median_np(x, off)[0])[table]
    for per_track, tab in ((1, L), (0, np.ascontiguousarray(L[7]))):
        want = R.apply_np(x, off, tab, symmetric)
        out = Guarded(x.shape, np.float32, 9.0)
        emul.emul_apply(vp(x), vp(off) if per_track else None, C.c_int64(N), P, vp(tab), per_track, symmetric, vp(out.a))
        assert same_bits(out.a, want), (per_track, where_differs(out.a, want))
        assert out.intact() and same_bits(x, keep)
        bad = ~R.frames_usable(x)
        assert bad.any() and same_bits(out.a[bad], x[bad])                              # NaN / Inf frames bit for bit
    if symmetric:
        assert same_bits(R.symmetric_np(R.symmetric_np(L)), R.symmetric_np(L))


def test_apply_copies_frames_of_no_track_through(emul):
    x, _ = R.median_tracks()
    x = np.ascontiguousarray(x[:200])
    off = np.array([10, 40, 40, 150], np.int64)
    L = R.median_np(x, off)[0]
    want = x.copy()
    want[10:150] = R.apply_np(x, off, L, 0)[10:150]
    out = Guarded(x.shape, np.float32, 9.0)
    emul.emul_apply(vp(x), vp(off), C.c_int64(len(x)), 3, vp(L), 1, 0, vp(out.a))
    assert same_bits(out.a, want) and out.intact()


class DeviceState:
    def __init__(self, state):
        self.len = Guarded(state["len"].shape, np.float32, state["len"])
        self.cnt = Guarded(state["cnt"].shape, np.int32, state["cnt"])
        self.owner = Guarded(state["owner"].shape, np.int32, state["owner"])

    def equals(self, state):
        live = state["cnt"] > 0                                                        # len means something only there
        return (np.array_equal(self.cnt.a, state["cnt"]) and np.array_equal(self.len.a.view(np.uint32)[live], state["len"].view(np.uint32)[live])
                and np.array_equal(self.owner.a, state["owner"]) and all(g.intact() for g in (self.len, self.cnt, self.owner)))


@pytest.mark.parametrize("symmetric", [0, 1])
@pytest.mark.parametrize("window", [1, 2, 5])
def test_push_kernel_source_follows_the_rule(emul, window, symmetric):
    S = 5
    state = R.new_state(S, fill=-7.0)
    dev = DeviceState(state)
    for i in range(14):
        slots = (None, np.array([3, 0], np.int32), np.array([1, S, 4, -1], np.int32))[i % 3]      # every slot; a subset; ids outside [0, S) copy through
        K = S if slots is None else len(slots)
        x = R.live_rows(i, K, seed=3)
        keep = x.copy()
        want = R.push_np(state, x, slots, window, symmetric)
        out = Guarded(x.shape, np.float32, 9.0)
        emul.emul_push(vp(x), vp(slots) if slots is not None else None, K, S, window, symmetric, vp(dev.len.a), vp(dev.cnt.a), vp(out.a))
        assert same_bits(out.a, want), (i, where_differs(out.a, want))
        assert dev.equals(state) and out.intact() and same_bits(x, keep), i
        if slots is not None and len(slots) == 4:
            assert same_bits(out.a[1], x[1]) and same_bits(out.a[3], x[3])
    assert state["cnt"].max() == window and (state["cnt"] > 0).all()


@pytest.mark.parametrize("rows,R_", [("persons", 2), ("tracks", 4)])
def test_tracked_kernel_source_follows_the_rule_and_the_one_euro_rows(emul, tmp_path_factory, rows, R_):
    """The tracked form over tracked_ref.script, every case of tracked_ref.Cases seen; row_slot equals smooth_ref.tracked_np's, and k_one_euro_tracked's own."""
    smooth = build(tmp_path_factory, "bones_smooth_host", "emul_smooth.cpp")
    n, window = B * R_, 3
    state, euro, cases = R.new_state(B * S_T, fill=-7.0), smooth_ref.new_state(B * S_T, 17, 3), Cases(T, S_T, R_)
    dev = DeviceState(state)
    p = smooth_ref.params()
    e_xhat, e_dxhat = np.zeros((B * S_T, 17, 3), np.float32), np.zeros((B * S_T, 17, 3), np.float32)
    e_last, e_owner = np.full((B * S_T, 17), -1, np.int64), np.zeros(B * S_T, np.int32)
    p_arr = np.array([p["dt"], p["min_cutoff"], p["d_cutoff"], p["beta"], p["min_score"]], np.float32)
    for i, arrays in enumerate(script(T, 3 * T + 4)):
        x = R.live_rows(i, n, seed=T)
        keep = x.copy()
        owner_before = state["owner"].copy()
        want, want_slot, reset, why = R.tracked_np(state, x, arrays, rows, R_, window, i % 2)
        cases.see(i, arrays, owner_before, state["owner"], state["count"], want_slot, reset, why)
        _, euro_slot, _, _ = smooth_ref.tracked_np(euro, p, x, arrays, rows, R_, i, False)
        assert np.array_equal(want_slot, euro_slot)
        out, row_slot = Guarded(x.shape, np.float32, 9.0), Guarded((n,), np.int32, -7)
        a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        emul.emul_tracked(vp(x), vp(a["ids"]), vp(a["slot"]), vp(a["born"]), vp(a["count"]), B, S_T, 0 if rows == "persons" else 1, R_, window, i % 2,
                          vp(dev.len.a), vp(dev.cnt.a), vp(dev.owner.a), vp(out.a), vp(row_slot.a) if i % 4 else None)
        assert same_bits(out.a, want), (i, where_differs(out.a, want))
        assert np.array_equal(row_slot.a, want_slot if i % 4 else np.full(n, -7, np.int32)), i
        assert dev.equals(state) and out.intact() and row_slot.intact() and same_bits(x, keep), i
        # the One-Euro kernel's own resolve over the same tick: the same row_slot and the same owner table
        e_out, e_slot = np.empty_like(x), np.full(n, -7, np.int32)
        smooth.emul_tracked(vp(x), vp(a["ids"]), vp(a["slot"]), vp(a["born"]), vp(a["count"]), B, S_T, 0 if rows == "persons" else 1, R_, 17, 3, 0, vp(p_arr),
                            p["max_hold"], C.c_int64(i), vp(e_xhat), vp(e_dxhat), vp(e_last), vp(e_owner), vp(e_out), vp(e_slot))
        assert np.array_equal(e_slot, want_slot) and np.array_equal(e_owner, dev.owner.a), i
    assert not cases.missing(), cases.missing()
    assert (state["cnt"] > 0).any()
