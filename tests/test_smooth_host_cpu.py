"""csrc/k_smooth.hip without a GPU: the kernels' own source compiled for the host with g++ behind a lockstep emulation of a workgroup (tests/host_emul/) and held
to the numpy restatement of include/kasf.h's rule (tests/smooth_ref.py) bit for bit: outputs, xhat / dxhat / last / owner after every tick, row_slot, canaries
around every array, inputs unchanged.  It shows the kernels' logic, their indexing and their fp32 operation order; what only the device can show stays with
tests/test_gpu_smooth.py."""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build, vp
from tests.smooth_ref import SHAPES, new_state, params, push_np, rows_for, tracked_np, tracks_np
from tests.tracked_ref import Cases, script

B, S_T, T = 2, 4, 5
PAD = 64


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build(tmp_path_factory, "smooth_host", "emul_smooth.cpp")


class Guarded:
    """An array with PAD canary elements on either side."""

    def __init__(self, shape, dtype, fill):
        n = int(np.prod(shape))
        self.canary = np.frombuffer(bytes([0x5A]) * np.dtype(dtype).itemsize, dtype)[0]
        self.buf = np.full(n + 2 * PAD, self.canary, dtype)
        self.a = self.buf[PAD:PAD + n].reshape(shape)
        self.a[...] = fill

    def intact(self):
        raw = self.buf.view(np.uint8)
        w = PAD * self.buf.itemsize
        c = np.frombuffer(self.canary.tobytes(), np.uint8)
        return bool((raw[:w].reshape(PAD, -1) == c).all() and (raw[len(raw) - w:].reshape(PAD, -1) == c).all())


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint64), b.view(np.uint32 if b.itemsize == 4 else np.uint64))


def p_array(p):
    return np.array([p["dt"], p["min_cutoff"], p["d_cutoff"], p["beta"], p["min_score"]], np.float32)


class DeviceState:
    """The kernel's side of a state: guarded copies of a restatement state."""

    def __init__(self, state):
        self.xhat, self.dxhat = (Guarded(state[k].shape, np.float32, state[k]) for k in ("xhat", "dxhat"))
        self.last = Guarded(state["last"].shape, np.int64, state["last"])
        self.owner = Guarded(state["owner"].shape, np.int32, state["owner"])

    def equals(self, state):
        return (same_bits(self.xhat.a, state["xhat"]) and same_bits(self.dxhat.a, state["dxhat"]) and np.array_equal(self.last.a, state["last"])
                and np.array_equal(self.owner.a, state["owner"]) and all(g.intact() for g in (self.xhat, self.dxhat, self.last, self.owner)))


@pytest.mark.parametrize("J,Cn,score", SHAPES)
@pytest.mark.parametrize("rows,R", [("persons", 2), ("tracks", 4)])
def test_tracked_kernel_source_follows_the_rule(emul, rows, R, J, Cn, score):
    p, n = params(min_score=0.3, max_hold=2), B * R
    state, cases = new_state(B * S_T, J, Cn, fill=-7.0), Cases(T, S_T, R)
    dev = DeviceState(state)
    tick = 0
    for i, arrays in enumerate(script(T, 3 * T + 4)):
        x = rows_for(i, n, J, Cn, score, seed=T)
        keep = x.copy()
        owner_before = state["owner"].copy()
        want, want_slot, reset, why = tracked_np(state, p, x, arrays, rows, R, tick, score)
        cases.see(i, arrays, owner_before, state["owner"], state["count"], want_slot, reset, why)
        out, row_slot = Guarded(x.shape, np.float32, 9.0), Guarded((n,), np.int32, -7)
        a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        emul.emul_tracked(vp(x), vp(a["ids"]), vp(a["slot"]), vp(a["born"]), vp(a["count"]), B, S_T, 0 if rows == "persons" else 1, R, J, Cn, int(score),
                          vp(p_array(p)), p["max_hold"], C.c_int64(tick), vp(dev.xhat.a), vp(dev.dxhat.a), vp(dev.last.a), vp(dev.owner.a), vp(out.a),
                          vp(row_slot.a) if i % 4 else None)
        assert same_bits(out.a, want), (i, np.argwhere(out.a.view(np.uint32) != want.view(np.uint32))[:4])
        assert np.array_equal(row_slot.a, want_slot if i % 4 else np.full(n, -7, np.int32)), i
        assert dev.equals(state) and out.intact() and row_slot.intact() and same_bits(x, keep), i
        tick += 3 if i == 7 else 1                                 # one tick is skipped twice over: k = 3 for every joint updated before it
    assert not cases.missing(), cases.missing()
    assert (state["last"] >= 0).any()


@pytest.mark.parametrize("J,Cn,score", SHAPES)
def test_push_kernel_source_follows_the_rule(emul, J, Cn, score):
    S, p = 5, params(min_score=0.3, max_hold=2)
    state = new_state(S, J, Cn, fill=-7.0)
    dev = DeviceState(state)
    tick = 0
    for i in range(14):
        slots = (None, np.array([3, 0], np.int32), np.array([1, S, 4, -1], np.int32))[i % 3]      # every slot; a subset; ids outside [0, S) copy through
        K = S if slots is None else len(slots)
        x = rows_for(i, K, J, Cn, score, seed=3)
        keep = x.copy()
        want = push_np(state, p, x, slots, tick, score)
        out = Guarded(x.shape, np.float32, 9.0)
        emul.emul_push(vp(x), vp(slots) if slots is not None else None, K, S, J, Cn, int(score), vp(p_array(p)), p["max_hold"], C.c_int64(tick), vp(dev.xhat.a),
                       vp(dev.dxhat.a), vp(dev.last.a), vp(out.a))
        assert same_bits(out.a, want), (i, np.argwhere(out.a.view(np.uint32) != want.view(np.uint32))[:4])
        assert dev.equals(state) and out.intact() and same_bits(x, keep), i
        if slots is not None and len(slots) == 4:
            assert same_bits(out.a[1], x[1]) and same_bits(out.a[3], x[3])
        tick += 3 if i == 8 else 1
    assert (state["last"] >= 0).any()



@pytest.mark.parametrize("J,Cn,score", SHAPES)
def test_tracks_kernel_source_equals_push_frame_by_frame(emul, J, Cn, score):
    p = params(min_score=0.3, max_hold=2)
    lengths = [0, 1, 2, 40]
    off = np.cumsum([0] + lengths).astype(np.int64)
    N, P = int(off[-1]), len(lengths)
    x = np.concatenate([rows_for(100 + f, 1, J, Cn, score, seed=9) for f in range(N)])
    keep = x.copy()
    out = Guarded(x.shape, np.float32, 9.0)
    emul.emul_tracks(vp(x), vp(off), C.c_int64(N), P, J, Cn, int(score), vp(p_array(p)), p["max_hold"], vp(out.a))
    assert out.intact() and same_bits(x, keep)
    assert same_bits(out.a, tracks_np(p, x, off, score))
    for t in range(P):                                             # the push kernel, frame by frame from an empty state
        dev = DeviceState(new_state(1, J, Cn))
        for tick, f in enumerate(range(off[t], off[t + 1])):
            o = np.empty((1, J, x.shape[2]), np.float32)
            emul.emul_push(vp(x[f:f + 1]), None, 1, 1, J, Cn, int(score), vp(p_array(p)), p["max_hold"], C.c_int64(tick), vp(dev.xhat.a), vp(dev.dxhat.a),
                           vp(dev.last.a), vp(o))
            assert same_bits(o[0], out.a[f]), (t, f)
