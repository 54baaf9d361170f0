"""csrc/k_stream_track.hip without a GPU: the kernels' own source compiled for the host with g++ behind a lockstep emulation of a workgroup
(tests/host_emul/: one host thread per GPU thread, a barrier at every __syncthreads / __syncthreads_or) and held to the numpy restatement of the tick rule
(tests/tracked_ref.py) and to numpy restatements of the clip and merge arithmetic, exactly.  It shows the kernels' logic, their indexing (canaries around every
array) and their fp32 / fp64 operation order; what only the device can show stays with tests/test_gpu_tracked.py.  T = 5 and a short run: 256 threads per row."""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build, vp
from tests.tracked_ref import Cases, frames_for, new_state, script, tracked_front_np

FLIP_SRC = [0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13]
B, S_T = 2, 4
RES = [(1280, 720), (1437, 913)]
CANARY = np.float32(12345.5)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build(tmp_path_factory, "tracked_host", "emul_tracked.cpp")


def clips_np(ring, count, slots, T, flip):
    """kasf_stream_windows in numpy for slots g of a [B*S_t] state, stream b = g // S_t: [(1+flip)*K, T, 17, 3]."""
    from kasportsformer_amd.stream import stream_tables
    r_tab = stream_tables(T)[0]
    out = []
    for g in slots:
        w_px, h_px = RES[g // S_T]
        k = max(int(count[g]), 1)
        L = min(k, T)
        f = np.clip(r_tab[L], 0, L - 1)
        c = ring[g][(k - L + f) % T]
        x = np.copy(c)
        scaled = (c[..., :2] / np.float32(w_px) * np.float32(2.0)).astype(np.float32)
        x[..., :2] = (scaled.astype(np.float64) - np.array([1.0, np.float64(np.float32(h_px)) / np.float64(np.float32(w_px))])).astype(np.float32)
        out.append(x)
    x = np.stack(out)
    if not flip:
        return x
    m = x[:, :, FLIP_SRC].copy()
    m[..., 0] = -m[..., 0]
    return np.concatenate((x, m))


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("rows,R", [("persons", 2), ("tracks", 4)])
def test_front_kernel_source_follows_the_rule(emul, rows, R, flip):
    from kasportsformer_amd.stream import stream_tables
    T, n, halves = 5, B * R, (2 if flip else 1)
    state, cases = new_state(B, S_T, T, fill=-1.0), Cases(T, S_T, R)
    ring_floats, x_floats = B * S_T * T * 51, halves * n * T * 51
    ring_buf = np.full(ring_floats + 128, CANARY, np.float32)
    ring = ring_buf[64:64 + ring_floats].reshape(B * S_T, T, 17, 3)
    ring[:] = -1.0
    count, owner = np.zeros(B * S_T, np.int64), np.zeros(B * S_T, np.int32)
    r_tab = np.ascontiguousarray(stream_tables(T)[0])
    w, h = np.array([r[0] for r in RES], np.float32), np.array([r[1] for r in RES], np.float32)
    for tick, arrays in enumerate(script(T, 3 * T + 4)):
        fr = frames_for(tick, n, seed=T)
        keep = fr.copy()
        owner_before = state["owner"].copy()
        want_slot, reset, why = tracked_front_np(state, arrays, rows, R, fr)
        cases.see(tick, arrays, owner_before, state["owner"], state["count"], want_slot, reset, why)
        x_buf = np.full(x_floats + 65, CANARY, np.float32)
        x = x_buf[1:1 + x_floats].reshape(halves * n, T, 17, 3)                  # clips at every alignment
        row_slot = np.full(n + 2, -7, np.int32)
        a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
        emul.emul_front(vp(fr), vp(a["ids"]), vp(a["slot"]), vp(a["born"]), vp(a["count"]), B, S_T, 0 if rows == "persons" else 1, R, T, vp(ring), vp(count),
                        vp(owner), vp(w), vp(h), vp(r_tab), int(flip), vp(x), vp(row_slot[1:]))
        assert np.array_equal(row_slot[1:-1], want_slot) and row_slot[0] == row_slot[-1] == -7, (tick, row_slot, want_slot)
        assert np.array_equal(count, state["count"]) and np.array_equal(owner, state["owner"]) and np.array_equal(ring, state["ring"]), tick
        assert np.array_equal(fr, keep)
        assert (ring_buf[:64] == CANARY).all() and (ring_buf[-64:] == CANARY).all() and x_buf[0] == CANARY and (x_buf[1 + x_floats:] == CANARY).all(), tick
        valid = [r for r in range(n) if want_slot[r] >= 0]
        if valid:
            xw = clips_np(ring, count, [int(want_slot[r]) for r in valid], T, flip)
            for hh in range(halves):
                for i, r in enumerate(valid):
                    assert np.array_equal(x[hh * n + r].view(np.uint32), xw[hh * len(valid) + i].view(np.uint32)), (tick, hh, r)
        for hh in range(halves):
            for r in range(n):
                if want_slot[r] < 0:
                    assert not x[hh * n + r].any(), (tick, hh, r)
    assert not cases.missing(), cases.missing()


@pytest.mark.parametrize("flip", [True, False])
def test_emit_kernel_source_merges_as_stream_emit(emul, flip):
    from kasportsformer_amd.stream import stream_tables
    T, halves = 5, (2 if flip else 1)
    fp_tab = np.ascontiguousarray(stream_tables(T)[1])
    count = np.array([1, 2, T - 1, T, T + 1, 2 * T + 3, 0, 3 * T + 5], np.int64)
    owner = np.array([3, 1, 4, 1, 5, 9, 2, 6], np.int32)
    row_slot = np.array([5, -1, 0, 3, -1, 7, 2, 4, 1], np.int32)
    n = len(row_slot)
    pred = np.random.default_rng(int(flip)).standard_normal((halves * n, T, 17, 3)).astype(np.float32)
    for back in (0, 3, T - 1):
        out = np.full((n + 1, 17, 3), CANARY, np.float32)
        valid, ids_out, frames_out = np.full(n + 1, 7, np.uint8), np.full(n + 1, -7, np.int32), np.full(n + 1, -7, np.int64)
        emul.emul_emit(vp(pred), int(flip), vp(count), vp(owner), vp(row_slot), C.c_int64(n), T, vp(fp_tab), back, vp(out), vp(valid), vp(ids_out), vp(frames_out))
        assert (out[n] == CANARY).all() and valid[n] == 7 and ids_out[n] == -7 and frames_out[n] == -7
        for r, g in enumerate(row_slot):
            if g < 0:
                assert not out[r].any() and valid[r] == 0 and ids_out[r] == 0 and frames_out[r] == 0, (back, r)
                continue
            L = min(max(int(count[g]), 1), T)
            t = fp_tab[L][min(max(L - 1 - back, 0), L - 1)]
            v = pred[r, t].copy()
            if flip:
                fv = pred[n + r, t][FLIP_SRC].copy()
                fv[:, 0] = -fv[:, 0]
                v = (v + fv) / np.float32(2)
            v[0] = 0
            assert np.array_equal(out[r].view(np.uint32), (np.float32(0) + v).view(np.uint32)), (back, r)
            assert valid[r] == 1 and ids_out[r] == owner[g] and frames_out[r] == count[g], (back, r)
