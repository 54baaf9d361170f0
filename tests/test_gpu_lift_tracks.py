"""Lifting many tracks of different lengths in one call (kasportsformer_amd.lift_tracks, kasf_lift_windows_ragged / kasf_lift_stitch_ragged):
both kernels bit-exact against tests/lift_ref.py's per-track restatements in the packed clip order and, for equal lengths, against the uniform kernels, the whole call against lift_track
track by track and against its parts, chunking, the reference demo's lifts (tests/golden/lift_e2e.npz), the call's contract and the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.lift_ref import H_PX, W_PX, _flip_np, _stitch_t, _track
from tests.test_gpu_lift import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
T = 27
LENGTHS = [61, 0, 1, 20, 26, 27, 28, 54, 0, 200, 13, 100]          # empty, shorter than T, k T, k T + r, long
RES = [(1280, 720), (1920, 1080), (3840, 2160), (1000, 1000), (1437, 913), (640, 480)]


def _tracks(lengths, seed):
    return [_track(1, n, seed=seed + 13 * p)[0] for p, n in enumerate(lengths)]


def _res(P):
    return [RES[p % len(RES)][0] for p in range(P)], [RES[p % len(RES)][1] for p in range(P)]


def _clips_np(kp, s, w_px, h_px):
    """test_gpu_lift._windows_np's clips of one [N,17,3] track (no mirror), normalised at w_px x h_px."""
    from kasportsformer_amd.lift import window_plan
    starts, lengths, r, _ = window_plan(kp.shape[0], T, s)
    clips = []
    for a, L in zip(starts, lengths):
        c = kp[a:a + L]
        if L < T:
            c = c[r]
        res = np.copy(c)
        res[..., :2] = c[..., :2] / w_px * 2 - [1, h_px / w_px]
        clips.append(res)
    return clips


def _windows_ragged_np(kps, s, ws, hs, flip):
    """Every track's clips in track order, then (flip) their mirrored copies: clip h * windows + win_first[p] + w."""
    x = np.stack([c for kp, w, h in zip(kps, ws, hs) for c in _clips_np(kp, s, w, h)])
    return np.concatenate((x, _flip_np(x))) if flip else x


def _stitch_ragged_t(pred, lengths, s, flip):
    """test_gpu_lift._stitch_t track by track, on the track's plain and mirrored clips."""
    from kasportsformer_amd.lift import ragged_plan
    wf = ragged_plan(lengths, T, s)[0].tolist()
    half = wf[-1]
    outs = [torch.zeros(0, 17, 3)]
    for p, n in enumerate(lengths):
        if n:
            a, b = wf[p], wf[p + 1]
            mine = torch.cat((pred[a:b], pred[half + a:half + b])) if flip else pred[a:b]
            outs.append(_stitch_t(mine, 1, n, T, s, flip)[0])
    return torch.cat(outs)


def _device_plan(lengths, s, ws, hs):
    from kasportsformer_amd.lift import ragged_plan
    wf, r, fp = ragged_plan(lengths, T, s)
    off = np.cumsum([0] + list(lengths), dtype=np.int64)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    return dict(off=d(off), wf=d(wf), r=d(r), fp=d(fp), w=d(np.asarray(ws, np.float32)), h=d(np.asarray(hs, np.float32)),
                frames=int(off[-1]), windows=int(wf[-1]))


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("s", [27, 9])
def test_windows_kernel_is_bit_exact(s, flip):
    from kasportsformer_amd import _lib
    from kasportsformer_amd.lift import window_plan
    lib = _lib.load()
    kps = _tracks(LENGTHS, seed=s)
    ws, hs = _res(len(kps))
    want = torch.from_numpy(_windows_ragged_np(kps, s, ws, hs, flip))
    pl = _device_plan(LENGTHS, s, ws, hs)
    packed = torch.from_numpy(np.concatenate(kps)).cuda()
    x = torch.full(tuple(want.shape), float("nan"), device="cuda")
    _lib.check(lib.kasf_lift_windows_ragged(ptr(packed), ptr(pl["off"]), ptr(pl["wf"]), len(kps), pl["frames"], pl["windows"], ptr(pl["w"]),
                                            ptr(pl["h"]), T, s, ptr(pl["r"]), int(flip), ptr(x), stream()))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), want)
    assert torch.equal(packed.cpu(), torch.from_numpy(np.concatenate(kps)))
    # each track's clips are what kasf_lift_windows writes for that track alone
    wf, halves = pl["wf"].tolist(), (2 if flip else 1)
    for p, kp in enumerate(kps):
        if kp.shape[0] == 0:
            continue
        starts, _, r, _ = window_plan(kp.shape[0], T, s)
        one = torch.empty((halves * len(starts), T, 17, 3), device="cuda")
        tr, r_dev = torch.from_numpy(kp).cuda(), (torch.from_numpy(r).cuda() if r is not None else None)
        _lib.check(lib.kasf_lift_windows(ptr(tr), 1, kp.shape[0], float(ws[p]), float(hs[p]), T, s, ptr(r_dev), int(flip), ptr(one), stream()))
        mine = torch.cat([x[h * pl["windows"] + wf[p]:h * pl["windows"] + wf[p + 1]] for h in range(halves)])
        assert torch.equal(mine, one), p


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("s", [27, 9])
def test_stitch_kernel_is_bit_exact(s, flip):
    from kasportsformer_amd import _lib
    pl = _device_plan(LENGTHS, s, *_res(len(LENGTHS)))
    g = torch.Generator().manual_seed(s + 2 * flip)
    pred = torch.randn(((2 if flip else 1) * pl["windows"], T, 17, 3), generator=g)
    want = _stitch_ragged_t(pred, LENGTHS, s, flip)
    pred_d = pred.cuda()
    out = torch.full((pl["frames"], 17, 3), float("nan"), device="cuda")
    _lib.check(_lib.load().kasf_lift_stitch_ragged(ptr(pred_d), int(flip), ptr(pl["off"]), ptr(pl["wf"]), len(LENGTHS), pl["frames"], pl["windows"],
                                                   T, s, ptr(pl["fp"]), ptr(out), stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    assert torch.equal(pred_d.cpu(), pred)


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("N,s", [(1, 5), (3, 5), (5, 5), (10, 5), (13, 5), (6, 2), (12, 2)])
def test_equal_lengths_give_the_uniform_kernels_bits(N, s, flip):
    """Three tracks of one length at one resolution, T = 5: the ragged launches write the bits of kasf_lift_windows / kasf_lift_stitch -- a few launches, no model."""
    from kasportsformer_amd import _lib
    from kasportsformer_amd.lift import ragged_plan, window_plan
    lib, P, T5, halves = _lib.load(), 3, 5, (2 if flip else 1)
    w_px, h_px = RES[(N + s) % len(RES)]
    _, _, r, fp = window_plan(N, T5, s)
    wf, r_tab, fp_tab = ragged_plan([N] * P, T5, s)
    windows = int(wf[-1])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None      # noqa: E731
    track, off, wf_d = d(_track(P, N, seed=N + s)), d(np.arange(P + 1, dtype=np.int64) * N), d(wf)
    ws, hs = d(np.full(P, w_px, np.float32)), d(np.full(P, h_px, np.float32))
    r_d, fp_d, r_tab_d, fp_tab_d = d(r), d(fp), d(r_tab), d(fp_tab)
    x_u, x_r = (torch.full((halves * windows, T5, 17, 3), float("nan"), device="cuda") for _ in range(2))
    _lib.check(lib.kasf_lift_windows(ptr(track), P, N, float(w_px), float(h_px), T5, s, ptr(r_d), int(flip), ptr(x_u), stream()))
    _lib.check(lib.kasf_lift_windows_ragged(ptr(track), ptr(off), ptr(wf_d), P, P * N, windows, ptr(ws), ptr(hs), T5, s, ptr(r_tab_d), int(flip), ptr(x_r),
                                            stream()))
    pred = torch.randn((halves * windows, T5, 17, 3), generator=torch.Generator().manual_seed(N + 2 * flip)).cuda()
    o_u, o_r = (torch.full((P, N, 17, 3), float("nan"), device="cuda") for _ in range(2))
    _lib.check(lib.kasf_lift_stitch(ptr(pred), int(flip), P, N, T5, s, ptr(fp_d), ptr(o_u), stream()))
    _lib.check(lib.kasf_lift_stitch_ragged(ptr(pred), int(flip), ptr(off), ptr(wf_d), P, P * N, windows, T5, s, ptr(fp_tab_d), ptr(o_r), stream()))
    torch.cuda.synchronize()
    assert torch.equal(x_r.view(torch.int32), x_u.view(torch.int32)) and not torch.isnan(x_u).any()
    assert torch.equal(o_r.view(torch.int32), o_u.view(torch.int32)) and not torch.isnan(o_u).any()


_MODELS = {}


def _model(cd):
    if cd not in _MODELS:
        _MODELS[cd] = make_pair(2, 27, cd)[1].eval()
    return _MODELS[cd]


@pytest.mark.parametrize("s", [27, 9])
def test_each_track_is_lift_track_of_it(s):
    """fp32: an eval forward computes every clip alone, so the batch a track's windows share with other tracks changes no bit of its poses."""
    import kasportsformer_amd as K
    m = _model("fp32")
    kps = _tracks(LENGTHS, seed=40 + s)
    ws, hs = _res(len(kps))
    got = K.lift_tracks(m, kps, ws, hs, stride=s)
    assert isinstance(got, list) and len(got) == len(kps)
    for p, kp in enumerate(kps):
        want = K.lift_track(m, kp, ws[p], hs[p], stride=s)
        assert got[p].is_cuda and got[p].dtype == torch.float32 and tuple(got[p].shape) == (kp.shape[0], 17, 3)
        assert torch.equal(got[p], want), p


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("s,flip", [(27, True), (9, True), (27, False)])
def test_lift_tracks_equals_forward_of_the_windows_bit_for_bit(s, flip, cd):
    """The whole call against its parts, no tolerance: the restated windows of every track in the packed clip order, one model forward of that
    stacked batch, and the restated stitch track by track."""
    import kasportsformer_amd as K
    m = _model(cd)
    kps = _tracks(LENGTHS, seed=70 + s)
    ws, hs = _res(len(kps))
    got = K.lift_tracks(m, kps, ws, hs, stride=s, flip=flip)
    with torch.no_grad():
        pred = m(torch.from_numpy(_windows_ragged_np(kps, s, ws, hs, flip)).cuda())
    want = _stitch_ragged_t(pred.cpu(), LENGTHS, s, flip)
    assert torch.equal(torch.cat(got).cpu(), want)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("P,N,s", [(3, 61, 27), (2, 100, 9), (4, 20, 27), (2, 54, 27)])
def test_equal_lengths_are_lift_track(P, N, s, cd):
    """Equal lengths: the packed clip order is lift_track's, so the forward sees the same batch -- bit-equal in both modes."""
    import kasportsformer_amd as K
    kp = _track(P, N, seed=5 + N)
    got = K.lift_tracks(_model(cd), list(kp), W_PX, H_PX, stride=s)
    want = K.lift_track(_model(cd), kp, W_PX, H_PX, stride=s)
    assert torch.equal(torch.stack(got), want)


@pytest.mark.parametrize("s", [27, 9])
def test_chunked_forward_equals_one_batch(s):
    import kasportsformer_amd as K
    m = _model("fp32")
    kps = _tracks(LENGTHS, seed=90)
    a = torch.cat(K.lift_tracks(m, kps, W_PX, H_PX, stride=s))
    for mw in (1, 2, 7):                                 # 7: chunk boundaries inside the 200- and the 100-frame track
        b = torch.cat(K.lift_tracks(m, kps, W_PX, H_PX, stride=s, max_windows=mw))
        assert torch.equal(a, b), mw


@pytest.mark.parametrize("cd,tol", [("fp32", 1e-3), ("bf16", 0.05)])
def test_one_call_matches_the_reference_demo(cd, tol):
    """Every track of the fixture (n1, n20, n27, n54, n61 and both persons of p2) in one ragged call, held to the bars of
    test_gpu_lift.test_lift_matches_the_reference_demo: the mode's tolerance on well-conditioned windows, the bf16 bar on the others."""
    import kasportsformer_amd as K
    from kasportsformer_amd.lift import window_plan
    fx = np.load(os.path.join(GOLDEN, "lift_e2e.npz"))
    cases = ["n1", "n20", "n27", "n54", "n61", "p2"]
    tracks, owner = [], []
    for c in cases:
        kp = fx["track_" + c]
        for person in (kp if kp.ndim == 4 else kp[None]):
            tracks.append(person)
            owner.append(c)
    got = K.lift_tracks(_model(cd), tracks, int(fx["width"]), int(fx["height"]))
    for c in cases:
        mine = torch.stack([g for g, o in zip(got, owner) if o == c]).cpu()
        want = torch.from_numpy(fx["lift_" + c]).reshape(mine.shape)
        assert torch.all(mine[..., 0, :] == 0)
        err = (mine - want).abs().amax(dim=(-2, -1)).reshape(-1) / want.abs().max()
        n = mine.shape[1]
        sens = torch.from_numpy(fx["sens_" + c]).reshape(-1, n)
        stable = torch.zeros_like(sens, dtype=torch.bool)
        starts, lengths, _, _ = window_plan(n, 27)
        for a, L in zip(starts, lengths):
            stable[:, a:a + L] = (sens[:, a:a + L].amax(dim=1) <= 1e-4)[:, None]
        stable = stable.reshape(-1)
        if c in ("n54", "n61"):
            assert stable.any(), "the fixture's tracks with full clips keep well-conditioned windows"
        if stable.any():
            assert err[stable].max() <= tol, (c, cd, err[stable].max().item())
        if (~stable).any():
            assert err[~stable].max() <= 0.05, (c, cd, err[~stable].max().item())


def test_input_mode_and_autograd_contract():
    import kasportsformer_amd as K
    m = make_pair(1, 27, "fp32")[1]
    kps = _tracks([40, 7, 0, 61], seed=9)
    copies = [k.copy() for k in kps]
    bufs = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    out = K.lift_tracks(m, kps, W_PX, H_PX)
    assert m.training, "the caller's training flag is restored"
    assert all(not o.requires_grad and o.grad_fn is None for o in out)
    assert all(np.array_equal(a, b) for a, b in zip(kps, copies))
    assert len({o.untyped_storage().data_ptr() for o in out}) == 1, "views of one packed result"
    # CPU tensors, GPU tensors, a mix of both with numpy, and the packed form: the same poses, inputs untouched
    cpu = [torch.from_numpy(k.copy()) for k in kps]
    dev = [torch.from_numpy(k).cuda() for k in kps]
    for inp in (cpu, dev, [dev[0], kps[1], cpu[2], dev[3]]):
        got = K.lift_tracks(m, inp, W_PX, H_PX)
        assert all(torch.equal(a, b) for a, b in zip(got, out))
    assert all(torch.equal(a, torch.from_numpy(b)) and torch.equal(d.cpu(), torch.from_numpy(b)) for a, d, b in zip(cpu, dev, copies))
    off = np.cumsum([0] + [len(k) for k in kps])
    packed_np = np.concatenate(kps)
    for packed, offsets in ((packed_np, off), (torch.from_numpy(packed_np).cuda(), torch.from_numpy(off).cuda())):
        got = K.lift_tracks(m, packed, W_PX, H_PX, offsets=offsets)
        assert isinstance(got, torch.Tensor) and torch.equal(got, torch.cat(out))
    assert np.array_equal(packed_np, np.concatenate(copies))
    for k, v in m.state_dict().items():                     # eval mode: no BatchNorm running-statistics update
        assert torch.equal(v, bufs[k]), k
    m.eval()
    assert K.lift_tracks(m, [], W_PX, H_PX) == []
    empty = K.lift_tracks(m, [np.zeros((0, 17, 3), np.float32)] * 3, W_PX, H_PX)
    assert len(empty) == 3 and all(e.is_cuda and tuple(e.shape) == (0, 17, 3) for e in empty)
    assert tuple(K.lift_tracks(m, np.zeros((0, 17, 3), np.float32), W_PX, H_PX, offsets=[0, 0]).shape) == (0, 17, 3)
    assert not m.training
    with pytest.raises(ValueError):
        K.lift_tracks(m, [np.zeros((5, 17, 2), np.float32)], W_PX, H_PX)
    with pytest.raises(ValueError):
        K.lift_tracks(m, [np.zeros((1, 5, 17, 3), np.float32)], W_PX, H_PX)
    with pytest.raises(TypeError):
        K.lift_tracks(m, [np.zeros((5, 17, 3), np.float64)], W_PX, H_PX)
    with pytest.raises(TypeError):
        K.lift_tracks(m, [[0.0] * 3], W_PX, H_PX)
    with pytest.raises(ValueError):
        K.lift_tracks(m, kps, W_PX, H_PX, stride=28)
    with pytest.raises(ValueError):
        K.lift_tracks(m, kps, [W_PX] * 3, H_PX)            # four tracks, three widths
    with pytest.raises(ValueError):
        K.lift_tracks(m, kps, W_PX, [H_PX, H_PX, -1, H_PX])
    with pytest.raises(ValueError):
        K.lift_tracks(m, kps, W_PX, H_PX, max_windows=0)
    for bad in (off[:-1], off[::-1], off.astype(np.float64), off[None]):
        with pytest.raises(ValueError):
            K.lift_tracks(m, packed_np, W_PX, H_PX, offsets=bad)
    with pytest.raises(RuntimeError):
        K.lift_tracks(m, [torch.zeros((5, 17, 3), device="meta")], W_PX, H_PX)
    with pytest.raises(RuntimeError):
        K.lift_tracks(make_pair(1, 27, "fp32")[1].cpu(), kps, W_PX, H_PX)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError):
            K.lift_tracks(m, [torch.zeros((5, 17, 3), device="cuda:1")], W_PX, H_PX)


def test_cli_writes_an_npz_of_what_lift_tracks_returns(tmp_path):
    """One fresh child process: yaml + checkpoint_save checkpoint + a pickled list of tracks -> .npz of track_i, bit for bit lift_tracks's output."""
    import yaml
    import kasportsformer_amd as K
    m = make_pair(1, 27, "fp32")[1].eval()
    cfg = {"model_name": "KASportsFormer", "n_layers": 1, "dim_in": 3, "dim_feat": 128, "dim_rep": 512, "dim_out": 3, "mlp_ratio": 4, "act_layer": "gelu",
           "attn_drop": 0.0, "drop": 0.0, "drop_path": 0.0, "use_layer_scale": True, "layer_scale_init_value": 0.00001, "use_adaptive_fusion": True,
           "num_heads": 8, "qkv_bias": False, "qkv_scale": None, "hierarchical": False, "num_joints": 17, "use_temporal_similarity": True,
           "neighbour_num": 4, "temporal_connection_len": 1, "use_tcn": False, "graph_only": False, "n_frames": 27}
    (tmp_path / "m.yaml").write_text(yaml.safe_dump(cfg))
    K.checkpoint_save(str(tmp_path / "best.pth"), 0, 1e-3, None, m, 100.0, "x")
    kps = _tracks([61, 5, 0, 30], seed=11)
    (tmp_path / "tracks.pkl").write_bytes(pickle.dumps(kps))
    cmd = [sys.executable, "-m", "kasportsformer_amd.lift", "--config", str(tmp_path / "m.yaml"), "--checkpoint", str(tmp_path / "best.pth"),
           "--keypoints", str(tmp_path / "tracks.pkl"), "--width", str(W_PX), "--height", str(H_PX), "--compute-dtype", "fp32", "--stride", "9",
           "--out", str(tmp_path / "poses3d.npz")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(tmp_path / "poses3d.npz")
    assert got.files == [f"track_{i}" for i in range(len(kps))]
    for i, w in enumerate(K.lift_tracks(m, kps, W_PX, H_PX, stride=9)):
        a, w = got[f"track_{i}"], w.cpu().numpy()
        assert a.dtype == np.float32 and a.shape == w.shape
        assert np.array_equal(a.view(np.uint32), w.view(np.uint32)), i
