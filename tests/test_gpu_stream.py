"""Lifting live keypoint streams frame by frame (kasportsformer_amd.StreamLifter, kasf_stream_push / _windows / _emit): the three kernels bit-exact
against the numpy / torch restatements of tests/lift_ref.py, the rule (every pose is lift_track of the slot's current window) tick by
tick, the call against its parts in both modes, replay against the rule and the reference demo's lifts (tests/golden/lift_e2e.npz), the contract
and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.lift_ref import H_PX, W_PX, _emit_t, _frames, _ring_state, _track, _windows_stream_np
from tests.test_gpu_lift import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
RES = [(1280, 720), (1920, 1080), (3840, 2160), (1000, 1000), (1437, 913), (640, 480), (800, 600)]


def _ks(T):
    return [1, 2, T - 1, T, T + 1, 2 * T, 3 * T + 5]


def _script(S, ticks, seed, always=()):
    """Per tick: None (every slot, in order) or a random subset of the slots in random order; slots in ``always`` are in every subset."""
    g = np.random.default_rng(seed)
    out = []
    for t in range(ticks):
        if t % 7 == 0:
            out.append(None)
            continue
        ids = [int(i) for i in g.permutation(S)[:int(g.integers(1, S + 1))]]
        out.append(ids + [a for a in always if a not in ids])
    return out


@pytest.mark.parametrize("T", [27, 81])
def test_push_kernel_matches_a_numpy_ring(T):
    from kasportsformer_amd import _lib
    lib = _lib.load()
    S, ticks = 5, 3 * T + 4
    ring = torch.full((S, T, 17, 3), -1.0, device="cuda")
    count = torch.zeros(S, dtype=torch.int64, device="cuda")
    ring_np, count_np = np.full((S, T, 17, 3), -1.0, np.float32), np.zeros(S, np.int64)
    for tick, ids in enumerate(_script(S, ticks, seed=T, always=(0,))):
        if ids is not None and T // 2 <= tick < T:                       # slot 2 is idle for a while
            ids = [i for i in ids if i != 2]
        if tick == 2 * T:                                               # slot 1 is reset mid-way: only its count is zeroed
            count[1] = 0
            count_np[1] = 0
        K = S if ids is None else len(ids)
        fr = _frames(K, seed=1000 * T + tick)
        fr_d = torch.from_numpy(fr).cuda()
        ids_d = torch.tensor(ids, dtype=torch.int32, device="cuda") if ids is not None else None
        _lib.check(lib.kasf_stream_push(ptr(fr_d), ptr(ids_d), K, S, T, ptr(ring), ptr(count), stream()))
        for i, s in enumerate(range(S) if ids is None else ids):
            ring_np[s, count_np[s] % T] = fr[i]
            count_np[s] += 1
        torch.cuda.synchronize()
        assert torch.equal(count.cpu(), torch.from_numpy(count_np)), tick
        assert torch.equal(ring.cpu(), torch.from_numpy(ring_np)), tick
        assert torch.equal(fr_d.cpu(), torch.from_numpy(fr)), tick
    assert count_np[0] == ticks > 3 * T and 0 < count_np[1] <= T + 4 and count_np[2] < ticks, "slot 0 wrapped three times; slot 2 idled, slot 1 restarted"


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("T", [27, 81])
def test_windows_kernel_is_bit_exact(T, flip):
    from kasportsformer_amd import _lib
    from kasportsformer_amd.lift import window_plan
    from kasportsformer_amd.stream import stream_tables
    lib = _lib.load()
    ks = _ks(T)
    S, halves = len(ks), (2 if flip else 1)
    hist, ring_np, count_np = _ring_state(T, ks, seed=T)
    ring, count = torch.from_numpy(ring_np).cuda(), torch.from_numpy(count_np).cuda()
    w_d = torch.tensor([RES[s][0] for s in range(S)], dtype=torch.float32, device="cuda")
    h_d = torch.tensor([RES[s][1] for s in range(S)], dtype=torch.float32, device="cuda")
    r_tab = torch.from_numpy(stream_tables(T)[0]).cuda()
    for ids in (None, [4, 0, 6, 3], [5], list(range(S))[::-1]):
        order = list(range(S)) if ids is None else ids
        K = len(order)
        windows = [hist[s][max(0, ks[s] - T):] for s in order]
        want = torch.from_numpy(_windows_stream_np(windows, T, [RES[s] for s in order], flip))
        ids_d = torch.tensor(ids, dtype=torch.int32, device="cuda") if ids is not None else None
        x = torch.full((halves * K, T, 17, 3), float("nan"), device="cuda")
        _lib.check(lib.kasf_stream_windows(ptr(ring), ptr(count), ptr(ids_d), K, S, T, ptr(w_d), ptr(h_d), ptr(r_tab), int(flip), ptr(x), stream()))
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), want), ids
        # ... and each slot's clips are what kasf_lift_windows writes for its current window alone
        for i, s in enumerate(order):
            w = windows[i]
            r = window_plan(len(w), T)[2]
            tr, r_dev = torch.from_numpy(np.ascontiguousarray(w)).cuda(), (torch.from_numpy(r).cuda() if r is not None else None)
            one = torch.empty((halves, T, 17, 3), device="cuda")
            _lib.check(lib.kasf_lift_windows(ptr(tr), 1, len(w), float(RES[s][0]), float(RES[s][1]), T, T, ptr(r_dev), int(flip), ptr(one), stream()))
            assert torch.equal(torch.stack([x[h * K + i] for h in range(halves)]), one), (ids, s)
    assert torch.equal(ring.cpu(), torch.from_numpy(ring_np)) and torch.equal(count.cpu(), torch.from_numpy(count_np))


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("T", [27, 81])
def test_emit_kernel_is_bit_exact(T, flip):
    from kasportsformer_amd import _lib
    from kasportsformer_amd.stream import stream_tables
    lib = _lib.load()
    ks = _ks(T)
    S, halves = len(ks), (2 if flip else 1)
    count = torch.tensor(ks, dtype=torch.int64, device="cuda")
    fp_tab = torch.from_numpy(stream_tables(T)[1]).cuda()
    for case, ids in enumerate((None, [6, 2, 0, 3, 1])):
        order = list(range(S)) if ids is None else ids
        K = len(order)
        Ls = [min(ks[s], T) for s in order]
        g = torch.Generator().manual_seed(T + 2 * flip + 10 * case)
        pred = torch.randn((halves * K, T, 17, 3), generator=g)
        pred_d = pred.cuda()
        ids_d = torch.tensor(ids, dtype=torch.int32, device="cuda") if ids is not None else None
        for back, n_out in ((0, 1), (5, 1), (T - 1, 1), (4, 5), (T - 2, T - 1)):
            want = _emit_t(pred, Ls, T, back, n_out, flip)
            out = torch.full((K, n_out, 17, 3), float("nan"), device="cuda")
            _lib.check(lib.kasf_stream_emit(ptr(pred_d), int(flip), ptr(count), ptr(ids_d), K, S, T, ptr(fp_tab), back, n_out, ptr(out), stream()))
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), want), (ids, back, n_out)
        assert torch.equal(pred_d.cpu(), pred)


_MODELS = {}


def _model(cd):
    if cd not in _MODELS:
        _MODELS[cd] = make_pair(2, 27, cd)[1].eval()
    return _MODELS[cd]


class _Forwards:
    """Counts the model's forward calls."""

    def __init__(self, model):
        self.n = 0
        self._h = model.register_forward_hook(lambda *a: setattr(self, "n", self.n + 1))

    def close(self):
        self._h.remove()


_REFS = {}


def _ref(m, hist_key, window, wh):
    """lift_track of one current window, [L,17,3]; the same window comes back for every lag."""
    import kasportsformer_amd as K
    if hist_key not in _REFS:
        _REFS[hist_key] = K.lift_track(m, np.ascontiguousarray(window), wh[0], wh[1])
    return _REFS[hist_key]


@pytest.mark.parametrize("lag", [0, 5, 26])
def test_every_pose_is_lift_track_of_the_current_window(lag):
    """fp32: 4 slots with their own resolutions, 70 ticks (slot 0 gets a frame in every one: its ring wraps twice), changing subsets, slot 1 reset at
    tick 40.  Every push row and every tail row against lift_track of the slot's current window; a second lifter fed the same histories in two calls
    per tick gives the same poses (an eval forward computes every clip alone)."""
    import kasportsformer_amd as K
    m, T, S = _model("fp32"), 27, 4
    ws, hs = [RES[s][0] for s in range(S)], [RES[s][1] for s in range(S)]
    a, b = K.StreamLifter(m, ws, hs, slots=S, lag=lag), K.StreamLifter(m, ws, hs, slots=S, lag=lag)
    hist, epoch = [[] for _ in range(S)], [0] * S
    fw = _Forwards(m)
    for tick, ids in enumerate(_script(S, 70, seed=3, always=(0,))):
        if tick == 40:
            a.reset(slots=[1])
            b.reset(slots=[1])
            hist[1], epoch[1] = [], 1
        order = list(range(S)) if ids is None else ids
        fr = _frames(len(order), seed=500 + tick)
        got = a.push(fr, slots=ids)
        half = len(order) // 2
        got_b = torch.cat([b.push(fr[:half], slots=order[:half]), b.push(fr[half:], slots=order[half:])])
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(order), 17, 3)
        assert torch.equal(got_b, got), tick
        for i, s in enumerate(order):
            hist[s].append(fr[i])
            k = len(hist[s])
            L = min(k, T)
            ref = _ref(m, (s, epoch[s], k), np.stack(hist[s][k - L:]), RES[s])
            assert torch.equal(got[i], ref[max(L - 1 - lag, 0)]), (tick, s, k)
        assert a.counts.tolist() == [len(h) for h in hist] == b.counts.tolist()
        if tick % 9 == 8 or tick == 69:
            live = [s for s in (3, 0, 2, 1) if hist[s]]
            before, n0 = a.counts, fw.n
            rest = a.tail(slots=live)
            assert tuple(rest.shape) == (len(live), lag, 17, 3) and fw.n == n0 + (1 if lag else 0)
            assert np.array_equal(a.counts, before)
            for i, s in enumerate(live):
                k = len(hist[s])
                L = min(k, T)
                ref = _ref(m, (s, epoch[s], k), np.stack(hist[s][k - L:]), RES[s])
                for r in range(lag):
                    assert torch.equal(rest[i, r], ref[min(max(L - lag + r, 0), L - 1)]), (tick, s, r)
    fw.close()
    assert len(hist[0]) == 70 and len(hist[1]) <= 30


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("flip,lag", [(True, 0), (True, 7), (False, 3)])
def test_push_equals_forward_of_the_windows_bit_for_bit(flip, lag, cd):
    """The tick against its parts, no tolerance: the restated current windows of the pushed slots in clip order, one model forward of that stacked
    batch, the restated emit.  60 ticks over 6 slots: warm-up windows, the first full one and wrapped rings, in both modes."""
    import kasportsformer_amd as K
    m, T, S = _model(cd), 27, 6
    lifter = K.StreamLifter(m, [RES[s][0] for s in range(S)], [RES[s][1] for s in range(S)], slots=S, flip=flip, lag=lag)
    hist = [[] for _ in range(S)]
    for tick, ids in enumerate(_script(S, 60, seed=11 + lag, always=(5,))):
        order = list(range(S)) if ids is None else ids
        fr = _frames(len(order), seed=900 + tick)
        got = lifter.push(fr, slots=ids)
        for i, s in enumerate(order):
            hist[s].append(fr[i])
        windows = [np.stack(hist[s][-T:]) for s in order]
        with torch.no_grad():
            pred = m(torch.from_numpy(_windows_stream_np(windows, T, [RES[s] for s in order], flip)).cuda())
        want = _emit_t(pred.cpu(), [len(w) for w in windows], T, lag, 1, flip)[:, 0]
        assert torch.equal(got.cpu(), want), tick
        if lag and tick % 10 == 9:
            live = [s for s in range(S) if hist[s]]
            windows = [np.stack(hist[s][-T:]) for s in live]
            with torch.no_grad():
                pred = m(torch.from_numpy(_windows_stream_np(windows, T, [RES[s] for s in live], flip)).cuda())
            assert torch.equal(lifter.tail(slots=live).cpu(), _emit_t(pred.cpu(), [len(w) for w in windows], T, lag - 1, lag, flip)), tick
    assert len(hist[5]) == 60


def _replay_rule(m, track, lag, T=27):
    """Frame f from the window after push number k = min(f + lag + 1, N): lift_track(track[max(0, k - T):k])[f - max(0, k - T)]."""
    import kasportsformer_amd as K
    N = track.shape[0]
    lifts, rows = {}, []
    for f in range(N):
        k = min(f + lag + 1, N)
        a = max(0, k - T)
        if k not in lifts:
            lifts[k] = K.lift_track(m, np.ascontiguousarray(track[a:k]), W_PX, H_PX)
        rows.append(lifts[k][f - a])
    return torch.stack(rows) if rows else torch.empty((0, 17, 3), device="cuda")


@pytest.mark.parametrize("lag", [0, 8, 26])
@pytest.mark.parametrize("N", [1, 20, 27, 28, 61])
def test_replay_is_the_rule_frame_by_frame(N, lag):
    import kasportsformer_amd as K
    m = _model("fp32")
    lifter = K.StreamLifter(m, W_PX, H_PX, slots=3, lag=lag)
    lifter.push(_frames(3, seed=1))                                     # live slots: replay leaves them alone
    ring, counts = lifter._ring.clone(), lifter.counts
    track = _frames(N, seed=60 + N)
    got = lifter.replay(track)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (N, 17, 3)
    assert torch.equal(got, _replay_rule(m, track, lag))
    if N <= 27 and lag == 26:
        assert torch.equal(got, K.lift_track(m, track, W_PX, H_PX))
    assert torch.equal(lifter._ring, ring) and np.array_equal(lifter.counts, counts)
    assert lifter._count.cpu().tolist() == counts.tolist()


def test_replay_of_two_tracks_and_of_nothing():
    import kasportsformer_amd as K
    m = _model("fp32")
    lifter = K.StreamLifter(m, W_PX, H_PX, slots=1, lag=8)
    tracks = _track(2, 61, seed=77)
    got = lifter.replay(tracks)
    assert tuple(got.shape) == (2, 61, 17, 3)
    for p in range(2):
        assert torch.equal(got[p], _replay_rule(m, tracks[p], 8)), p
    assert torch.equal(lifter.replay(torch.from_numpy(tracks).cuda()), got)
    assert tuple(lifter.replay(np.zeros((0, 17, 3), np.float32)).shape) == (0, 17, 3)
    assert tuple(lifter.replay(np.zeros((2, 0, 17, 3), np.float32)).shape) == (2, 0, 17, 3)
    # one resolution per slot: replay needs the recorded track's own
    per_slot = K.StreamLifter(m, [W_PX, 1920], [H_PX, 1080], slots=2, lag=8)
    with pytest.raises(ValueError):
        per_slot.replay(tracks[0])
    assert torch.equal(per_slot.replay(tracks[0], width=W_PX, height=H_PX), got[0])


@pytest.mark.parametrize("cd,tol", [("fp32", 1e-3), ("bf16", 0.05)])
@pytest.mark.parametrize("case", ["n1", "n20", "n27"])
def test_replay_matches_the_reference_demo(case, cd, tol):
    """lag = T - 1 on a track of at most T frames is the demo's own lift of it: held to test_gpu_lift.test_lift_matches_the_reference_demo's bars (the
    mode's tolerance where the fixture's sens_* says the reference's lift is well-conditioned, the bf16 bar elsewhere), and equal to lift_track."""
    import kasportsformer_amd as K
    from kasportsformer_amd.lift import window_plan
    fx = np.load(os.path.join(GOLDEN, "lift_e2e.npz"))
    kp, want = fx["track_" + case], fx["lift_" + case]
    lifter = K.StreamLifter(_model(cd), int(fx["width"]), int(fx["height"]), slots=1, lag=26)
    got = lifter.replay(kp)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert torch.all(got[..., 0, :] == 0)
    assert torch.equal(got, K.lift_track(_model(cd), kp, int(fx["width"]), int(fx["height"])))
    want = torch.from_numpy(want)
    err = (got.cpu() - want).abs().amax(dim=(-2, -1)).reshape(-1) / want.abs().max()
    sens = torch.from_numpy(fx["sens_" + case]).reshape(-1, kp.shape[-3])
    stable = torch.zeros_like(sens, dtype=torch.bool)
    starts, lengths, _, _ = window_plan(kp.shape[-3], 27)
    for a, L in zip(starts, lengths):
        stable[:, a:a + L] = (sens[:, a:a + L].amax(dim=1) <= 1e-4)[:, None]
    stable = stable.reshape(-1)
    if stable.any():
        assert err[stable].max() <= tol, (case, cd, err[stable].max().item())
    if (~stable).any():
        assert err[~stable].max() <= 0.05, (case, cd, err[~stable].max().item())


def test_input_mode_and_autograd_contract():
    import kasportsformer_amd as K
    m = make_pair(1, 27, "fp32")[1]
    S = 4
    bufs = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    lifters = [K.StreamLifter(m, W_PX, H_PX, slots=S, lag=2) for _ in range(3)]
    assert all(lf.counts.tolist() == [0] * S and lf.counts.dtype == np.int64 for lf in lifters)
    pushes = np.zeros(S, np.int64)
    for tick, ids in enumerate([None, [2, 0], [3], None, [1, 3, 0]]):
        K_ = S if ids is None else len(ids)
        fr = _frames(K_, seed=tick)
        keep = fr.copy()
        as_cpu, as_dev = torch.from_numpy(fr.copy()), torch.from_numpy(fr).cuda()
        outs = [lf.push(inp, slots=sl) for lf, inp, sl in zip(lifters, (fr, as_cpu, as_dev), (ids, None if ids is None else np.asarray(ids),
                                                                                               None if ids is None else torch.tensor(ids)))]
        assert all(o.is_cuda and o.dtype == torch.float32 and not o.requires_grad and o.grad_fn is None for o in outs)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        assert np.array_equal(fr, keep) and torch.equal(as_cpu, torch.from_numpy(keep)) and torch.equal(as_dev.cpu(), torch.from_numpy(keep))
        assert m.training, "the caller's training flag is restored"
        pushes[list(range(S)) if ids is None else ids] += 1
        assert all(np.array_equal(lf.counts, pushes) for lf in lifters)
    lf = lifters[0]
    assert lf._count.cpu().tolist() == pushes.tolist(), "the host mirror is the device's count"
    rest = lf.tail()
    assert tuple(rest.shape) == (S, 2, 17, 3) and rest.grad_fn is None and m.training
    for k, v in m.state_dict().items():                     # eval mode: no BatchNorm running-statistics update
        assert torch.equal(v, bufs[k]), k
    m.eval()
    empty = lf.push(np.zeros((0, 17, 3), np.float32), slots=[])
    assert empty.is_cuda and tuple(empty.shape) == (0, 17, 3) and not m.training
    lf.reset(slots=[1])
    pushes[1] = 0
    assert np.array_equal(lf.counts, pushes) and lf._count.cpu().tolist() == pushes.tolist()

    # refusals: raised before any kernel runs, the state stays as it was
    ring, count = lf._ring.clone(), lf._count.clone()
    fr = _frames(S, seed=99)
    bad = [
        (ValueError, lambda: lf.tail(slots=[1])),                                   # a slot without frames has no window
        (ValueError, lambda: lf.tail()),
        (ValueError, lambda: lf.push(fr[:2], slots=[2, 2])),                        # duplicate ids
        (ValueError, lambda: lf.push(fr[:2], slots=[0, S])),                        # out of range
        (ValueError, lambda: lf.push(fr[:2], slots=[0, -1])),
        (ValueError, lambda: lf.push(fr[:2], slots=[0.0, 1.0])),                    # ids are integers
        (ValueError, lambda: lf.push(fr[:2], slots=[[0, 1]])),
        (ValueError, lambda: lf.push(fr[:3], slots=[0, 1])),                        # one frame per pushed slot
        (ValueError, lambda: lf.push(fr[:2])),                                      # without ids: one frame for every slot
        (ValueError, lambda: lf.push(fr[:, :, :2])),
        (ValueError, lambda: lf.push(fr[None])),
        (TypeError, lambda: lf.push(fr.astype(np.float64))),
        (TypeError, lambda: lf.push(fr.tolist())),
        (RuntimeError, lambda: lf.push(torch.zeros((S, 17, 3), device="meta"))),
        (RuntimeError, lambda: lf.push(fr[:1], slots=torch.tensor([0]).cuda())),    # ids are host integers
        (ValueError, lambda: lf.reset(slots=[S])),
        (ValueError, lambda: lf.replay(fr[:, :, :2])),
        (TypeError, lambda: lf.replay(fr.astype(np.float64))),
        (ValueError, lambda: lf.replay(fr, width=W_PX)),
        (ValueError, lambda: lf.replay(fr, width=-1, height=H_PX)),
    ]
    if torch.cuda.device_count() > 1:
        bad.append((RuntimeError, lambda: lf.push(torch.zeros((S, 17, 3), device="cuda:1"))))
    for exc, call in bad:
        with pytest.raises(exc):
            call()
        assert np.array_equal(lf.counts, pushes)
        assert torch.equal(lf._ring, ring) and torch.equal(lf._count, count)
    for kw in (dict(lag=-1), dict(lag=27), dict(slots=0), dict(width=0), dict(height=-720), dict(width=[W_PX] * 3), dict(height=[H_PX, H_PX, 0, H_PX])):
        args = dict(width=W_PX, height=H_PX, slots=S)
        args.update(kw)
        with pytest.raises(ValueError):
            K.StreamLifter(m, **args)
    assert K.StreamLifter(m, W_PX, H_PX, slots=S, lag=26).lag == 26
    with pytest.raises(RuntimeError):
        K.StreamLifter(make_pair(1, 27, "fp32")[1].cpu(), W_PX, H_PX)


def test_cli_online_writes_what_replay_returns(tmp_path):
    """One fresh child process: --online --lag 8 writes, bit for bit, StreamLifter(..., lag=8).replay of the file; --online with --stride is refused."""
    import pickle
    import yaml
    import kasportsformer_amd as K
    m = make_pair(1, 27, "fp32")[1].eval()
    cfg = {"model_name": "KASportsFormer", "n_layers": 1, "dim_in": 3, "dim_feat": 128, "dim_rep": 512, "dim_out": 3, "mlp_ratio": 4, "act_layer": "gelu",
           "attn_drop": 0.0, "drop": 0.0, "drop_path": 0.0, "use_layer_scale": True, "layer_scale_init_value": 0.00001, "use_adaptive_fusion": True,
           "num_heads": 8, "qkv_bias": False, "qkv_scale": None, "hierarchical": False, "num_joints": 17, "use_temporal_similarity": True,
           "neighbour_num": 4, "temporal_connection_len": 1, "use_tcn": False, "graph_only": False, "n_frames": 27}
    (tmp_path / "m.yaml").write_text(yaml.safe_dump(cfg))
    K.checkpoint_save(str(tmp_path / "best.pth"), 0, 1e-3, None, m, 100.0, "x")
    kp = _track(2, 40, seed=11)
    (tmp_path / "keypoints2d.pkl").write_bytes(pickle.dumps(kp))
    tracks = [_frames(n, seed=20 + n) for n in (33, 5, 0)]
    (tmp_path / "tracks.pkl").write_bytes(pickle.dumps(tracks))
    base = [sys.executable, "-m", "kasportsformer_amd.lift", "--config", str(tmp_path / "m.yaml"), "--checkpoint", str(tmp_path / "best.pth"),
            "--width", str(W_PX), "--height", str(H_PX), "--compute-dtype", "fp32", "--online"]
    r = subprocess.run(base + ["--keypoints", str(tmp_path / "keypoints2d.pkl"), "--lag", "8", "--out", str(tmp_path / "poses3d.npy")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lifter = K.StreamLifter(m, W_PX, H_PX, slots=1, lag=8)
    got, want = np.load(tmp_path / "poses3d.npy"), lifter.replay(kp).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (2, 40, 17, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    r = subprocess.run(base + ["--keypoints", str(tmp_path / "tracks.pkl"), "--lag", "8", "--out", str(tmp_path / "poses3d.npz")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(tmp_path / "poses3d.npz")
    assert z.files == [f"track_{i}" for i in range(len(tracks))]
    for i, t in enumerate(tracks):
        w = lifter.replay(t).cpu().numpy()
        assert z[f"track_{i}"].shape == w.shape and np.array_equal(z[f"track_{i}"].view(np.uint32), w.view(np.uint32)), i
    r = subprocess.run(base + ["--keypoints", str(tmp_path / "keypoints2d.pkl"), "--stride", "9", "--out", str(tmp_path / "no.npy")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and not (tmp_path / "no.npy").exists()
