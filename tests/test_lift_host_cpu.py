"""csrc/k_lift.hip without a GPU: the kernels' own source (and csrc/lift_math.h, where their arithmetic lives) compiled for the host with g++ behind
tests/host_emul/'s lockstep emulation of a workgroup, and the seven launches held bit for bit to the numpy / torch restatements of tests/lift_ref.py.
It shows the kernels' logic, their indexing (canaries around every output) and their fp32 / fp64 operation order; what only the device can show stays
with tests/test_gpu_lift.py, test_gpu_lift_tracks.py and test_gpu_stream.py.  T = 5: the smallest clip length at which every branch of the plan exists."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.host_emul import build
from tests.lift_ref import H_PX, W_PX, _clip_np, _emit_t, _flip_np, _frames, _ring_state, _stitch_t, _track, _windows_np, _windows_stream_np

T = 5
RES = [(1280, 720), (1920, 1080), (3840, 2160), (1000, 1000), (1437, 913), (640, 480), (800, 600)]
CANARY = np.float32(12345.5)
PAD = 64
P_, I, L, F = C.c_void_p, C.c_int, C.c_int64, C.c_float
ARGS = {"emul_lift_windows": [P_, I, L, F, F, I, I, P_, I, P_], "emul_lift_stitch": [P_, I, I, L, I, I, P_, P_],
        "emul_lift_windows_ragged": [P_, L, P_, P_, I, L, P_, P_, I, I, P_, I, P_], "emul_lift_stitch_ragged": [P_, I, L, P_, P_, I, L, I, I, P_, P_],
        "emul_stream_push": [P_, P_, I, I, I, P_, P_], "emul_stream_windows": [P_, P_, P_, I, I, I, P_, P_, P_, I, P_],
        "emul_stream_emit": [P_, I, P_, P_, I, I, I, P_, I, I, P_]}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "lift_host", "emul_lift.cpp")
    for name, args in ARGS.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, None
    return lib


def vp(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


class Out:
    """A float32 output array of the given shape between two runs of canaries."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = np.full(n + 2 * PAD, CANARY, np.float32)
        self.a = self.buf[PAD:PAD + n].reshape(shape)
        self.a[:] = np.nan

    def intact(self):
        return (self.buf[:PAD] == CANARY).all() and (self.buf[PAD + self.a.size:] == CANARY).all()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _plan(n, s):
    from kasportsformer_amd.lift import window_plan
    return window_plan(n, T, s)


def windows_one(emul, kp, s, flip, w_px, h_px):
    """The uniform launch over kp [P,N,17,3]: x [(1+flip)*P*W, T, 17, 3]."""
    starts, _, r, _ = _plan(kp.shape[1], s)
    x = Out(((2 if flip else 1) * kp.shape[0] * len(starts), T, 17, 3))
    keep = kp.copy()
    emul.emul_lift_windows(vp(kp), kp.shape[0], kp.shape[1], w_px, h_px, T, s, vp(r), int(flip), vp(x.a))
    assert x.intact() and np.array_equal(kp, keep)
    return x.a


def stitch_one(emul, pred, P, n, s, flip):
    """The uniform launch over pred [(1+flip)*P*W, T, 17, 3]: out [P,n,17,3]."""
    out = Out((P, n, 17, 3))
    emul.emul_lift_stitch(vp(pred), int(flip), P, n, T, s, vp(_plan(n, s)[3]), vp(out.a))
    assert out.intact()
    return out.a


UNIFORM = [(1, 1, 5), (2, 3, 5), (1, 5, 5), (1, 10, 5), (2, 13, 5), (2, 12, 2), (1, 6, 1)]


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("P,N,s", UNIFORM)
def test_uniform_kernel_source_is_bit_exact(emul, P, N, s, flip):
    kp = _track(P, N, seed=N + 7 * P)
    assert same(windows_one(emul, kp, s, flip, W_PX, H_PX), _windows_np(kp, T, s, flip))
    W = len(_plan(N, s)[0])
    pred = torch.randn(((2 if flip else 1) * P * W, T, 17, 3), generator=torch.Generator().manual_seed(N * 31 + P))
    assert same(stitch_one(emul, pred.numpy(), P, N, s, flip), _stitch_t(pred, P, N, T, s, flip).numpy())


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("lengths,s", [([0, 1, 3, 5, 10, 13], 5), ([12, 6, 5, 2], 2)])
def test_ragged_kernel_source_is_bit_exact_and_each_track_is_the_uniform_launch(emul, lengths, s, flip):
    from kasportsformer_amd.lift import ragged_plan
    P, halves = len(lengths), (2 if flip else 1)
    res = [RES[p % 2] for p in range(P)]                                                        # two resolutions
    ws, hs = np.array([r[0] for r in res], np.float32), np.array([r[1] for r in res], np.float32)
    kps = [_track(1, n, seed=s + 13 * p)[0] for p, n in enumerate(lengths)]
    wf, r_tab, fp_tab = ragged_plan(lengths, T, s)
    off = np.cumsum([0] + lengths, dtype=np.int64)
    frames, windows = int(off[-1]), int(wf[-1])
    packed = np.concatenate(kps)
    x = Out((halves * windows, T, 17, 3))
    emul.emul_lift_windows_ragged(vp(packed), frames, vp(off), vp(wf), P, windows, vp(ws), vp(hs), T, s, vp(r_tab), int(flip), vp(x.a))
    assert x.intact() and np.array_equal(packed, np.concatenate(kps))
    plain = np.stack([_clip_np(kp[a:a + n], T, *wh) for kp, wh in zip(kps, res) for a, n in zip(*_plan(len(kp), s)[:2])])
    assert same(x.a, np.concatenate((plain, _flip_np(plain))) if flip else plain)
    pred = torch.randn((halves * windows, T, 17, 3), generator=torch.Generator().manual_seed(s + 2 * flip))
    out = Out((frames, 17, 3))
    emul.emul_lift_stitch_ragged(vp(pred.numpy()), int(flip), windows, vp(off), vp(wf), P, frames, T, s, vp(fp_tab), vp(out.a))
    assert out.intact()
    for p, n in enumerate(lengths):
        if n == 0:
            continue
        rows = [slice(h * windows + wf[p], h * windows + wf[p + 1]) for h in range(halves)]
        assert same(np.concatenate([x.a[i] for i in rows]), windows_one(emul, kps[p][None], s, flip, *res[p])), p
        mine = torch.cat([pred[i] for i in rows])
        assert same(out.a[off[p]:off[p + 1]], _stitch_t(mine, 1, n, T, s, flip)[0].numpy()), p
        assert same(out.a[off[p]:off[p + 1]], stitch_one(emul, mine.numpy(), 1, n, s, flip)[0]), p


KS = [1, 2, 4, 5, 6, 10, 20]
ORDERS = [None, [4, 0, 6, 3, 1]]


@pytest.mark.parametrize("flip", [True, False])
def test_stream_windows_and_emit_kernel_source_is_bit_exact(emul, flip):
    from kasportsformer_amd.stream import stream_tables
    S, halves = len(KS), (2 if flip else 1)
    hist, ring, count = _ring_state(T, KS, seed=T)
    ring_keep = ring.copy()
    r_tab, fp_tab = stream_tables(T)
    ws, hs = np.array([r[0] for r in RES], np.float32), np.array([r[1] for r in RES], np.float32)
    for case, ids in enumerate(ORDERS):
        order = list(range(S)) if ids is None else ids
        K, ids_a = len(order), (None if ids is None else np.asarray(ids, np.int32))
        windows = [hist[s][max(0, KS[s] - T):] for s in order]
        x = Out((halves * K, T, 17, 3))
        emul.emul_stream_windows(vp(ring), vp(count), vp(ids_a), K, S, T, vp(ws), vp(hs), vp(r_tab), int(flip), vp(x.a))
        assert x.intact() and same(x.a, _windows_stream_np(windows, T, [RES[s] for s in order], flip)), ids
        for i, s in enumerate(order):                                                           # ... and what the uniform launch writes for that window alone
            one = windows_one(emul, np.ascontiguousarray(windows[i])[None], T, flip, *RES[s])
            assert same(np.stack([x.a[h * K + i] for h in range(halves)]), one), (ids, s)
        pred = torch.randn((halves * K, T, 17, 3), generator=torch.Generator().manual_seed(T + 2 * flip + 10 * case))
        for back, n_out in ((0, 1), (2, 1), (4, 1), (2, 3)):
            out = Out((K, n_out, 17, 3))
            emul.emul_stream_emit(vp(pred.numpy()), int(flip), vp(count), vp(ids_a), K, S, T, vp(fp_tab), back, n_out, vp(out.a))
            assert out.intact() and same(out.a, _emit_t(pred, [min(KS[s], T) for s in order], T, back, n_out, flip).numpy()), (ids, back, n_out)
    assert np.array_equal(ring, ring_keep) and count.tolist() == KS


def test_stream_push_kernel_source_matches_a_numpy_ring(emul):
    S, ticks = 4, 3 * T + 4
    ring, count = Out((S, T, 17, 3)), np.zeros(S + 2, np.int64)
    ring.a[:] = -1.0
    count[0] = count[-1] = -7
    ring_np, count_np = np.full((S, T, 17, 3), -1.0, np.float32), np.zeros(S, np.int64)
    g = np.random.default_rng(T)
    for tick in range(ticks):
        ids = None if tick % 7 == 0 else sorted({0, *g.permutation(S)[:int(g.integers(1, S + 1))].tolist()}, key=lambda s: (s * 7 + tick) % S)
        if tick == 2 * T:                                                                       # slot 1 is reset mid-way: only its count is zeroed
            count[2] = count_np[1] = 0
        order = list(range(S)) if ids is None else ids
        fr = _frames(len(order), seed=1000 * T + tick)
        keep = fr.copy()
        emul.emul_stream_push(vp(fr), vp(None if ids is None else np.asarray(ids, np.int32)), len(order), S, T, vp(ring.a), vp(count[1:]))
        for i, s in enumerate(order):
            ring_np[s, count_np[s] % T] = fr[i]
            count_np[s] += 1
        assert ring.intact() and same(ring.a, ring_np) and np.array_equal(count[1:-1], count_np) and count[0] == count[-1] == -7, tick
        assert np.array_equal(fr, keep)
    assert count_np[0] == ticks > 3 * T and 0 < count_np[1] <= T + 4
