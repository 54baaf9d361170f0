"""Lifting a 2-D keypoint track to 3-D on the GPU (kasportsformer_amd.lift_track, kasf_lift_windows / kasf_lift_stitch): both kernels
bit-exact against restatements of the demo's arithmetic (demo/demo.py:132-156,222-236, demo/lib/utils.py:5-20), the whole lift against
the reference demo's own per-clip loop (tests/golden/lift_e2e.npz), chunking, the call's contract and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.lift_ref import H_PX, W_PX, _stitch_t, _track, _windows_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [(1, 1, 27, 27), (1, 20, 27, 27), (2, 61, 27, 27), (1, 54, 27, 27), (3, 200, 81, 81), (2, 100, 27, 9), (1, 30, 27, 9),
         (1, 28, 27, 1), (2, 20, 27, 9), (1, 300, 81, 27)]


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("P,N,T,s", CASES)
def test_windows_kernel_is_bit_exact(P, N, T, s, flip):
    from kasportsformer_amd import _lib
    from kasportsformer_amd.lift import window_plan
    kp = _track(P, N, seed=N + 7 * P)
    want = torch.from_numpy(_windows_np(kp, T, s, flip))
    _, _, r, _ = window_plan(N, T, s)
    track = torch.from_numpy(kp).cuda()
    r_dev = torch.from_numpy(r).cuda() if r is not None else None
    x = torch.full(tuple(want.shape), float("nan"), device="cuda")
    _lib.check(_lib.load().kasf_lift_windows(ptr(track), P, N, float(W_PX), float(H_PX), T, s, ptr(r_dev), int(flip), ptr(x), stream()))
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), want)
    assert torch.equal(track.cpu(), torch.from_numpy(kp))


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("P,N,T,s", CASES)
def test_stitch_kernel_is_bit_exact(P, N, T, s, flip):
    from kasportsformer_amd import _lib
    from kasportsformer_amd.lift import window_plan
    starts, _, _, fp = window_plan(N, T, s)
    W = len(starts)
    g = torch.Generator().manual_seed(N * 31 + P)
    pred = torch.randn(((2 if flip else 1) * P * W, T, 17, 3), generator=g)
    want = _stitch_t(pred, P, N, T, s, flip)
    pred_d = pred.cuda()
    fp_dev = torch.from_numpy(fp).cuda() if fp is not None else None
    out = torch.full((P, N, 17, 3), float("nan"), device="cuda")
    _lib.check(_lib.load().kasf_lift_stitch(ptr(pred_d), int(flip), P, N, T, s, ptr(fp_dev), ptr(out), stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)


_MODELS = {}


def _model(cd):
    if cd not in _MODELS:
        _MODELS[cd] = make_pair(2, 27, cd)[1].eval()
    return _MODELS[cd]


@pytest.mark.parametrize("cd,tol", [("fp32", 1e-3), ("bf16", 0.05)])
@pytest.mark.parametrize("case", ["n1", "n20", "n27", "n54", "n61", "p2"])
def test_lift_matches_the_reference_demo(case, cd, tol):
    """The demo's lift (flip on a copy; N = 54 from full clips, where turn_into_clips raises) with the real reference model, 2 layers.
    Windows hold the mode's bar where the reference's lift is well-conditioned.  The fixture's sens_* records, per frame, how far the reference's
    OWN lift moves when the pixel track carries 1e-6 relative noise (eight draws): 2e-6 .. 1e-4 on 6 of the 12 person-windows (two resampled
    tails among them), 1.7e-4 .. 7.1e-3 on the other 6 -- near-ties in the temporal GCN's top-k similarities (graph.py:104-112) of this
    random-weight model.  In such a window any rounding difference may pick another neighbour, and the change spreads over the window (the
    CPU oracle, run on all windows of n61 as one batch rather than clip by clip, differs from the fixture by 7e-3 on frames 27, 29 and 49),
    so a window with any frame above 1e-4 is held to the bf16 bar in both modes.  test_lift_equals_forward_of_the_windows_bit_for_bit holds
    every window, resampled and mirrored ones included, to exact equality with the forward it runs."""
    import kasportsformer_amd as K
    fx = np.load(os.path.join(GOLDEN, "lift_e2e.npz"))
    kp, want = fx["track_" + case], fx["lift_" + case]
    got = K.lift_track(_model(cd), kp, int(fx["width"]), int(fx["height"]))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert torch.all(got[..., 0, :] == 0)
    want = torch.from_numpy(want)
    err = (got.cpu() - want).abs().amax(dim=(-2, -1)).reshape(-1) / want.abs().max()     # per frame, relative to the whole lift's scale
    from kasportsformer_amd.lift import window_plan
    sens = torch.from_numpy(fx["sens_" + case]).reshape(-1, kp.shape[-3])
    stable = torch.zeros_like(sens, dtype=torch.bool)
    starts, lengths, _, _ = window_plan(kp.shape[-3], 27)
    for a, L in zip(starts, lengths):
        stable[:, a:a + L] = (sens[:, a:a + L].amax(dim=1) <= 1e-4)[:, None]
    stable = stable.reshape(-1)
    if case in ("n54", "n61"):
        assert stable.any(), "the fixture's tracks with full clips keep well-conditioned windows"
    if stable.any():
        assert err[stable].max() <= tol, (case, cd, err[stable].max().item())
    if (~stable).any():
        assert err[~stable].max() <= 0.05, (case, cd, err[~stable].max().item())


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("P,N,s,flip,mw", [(1, 61, 27, True, 1024), (2, 40, 27, True, 1024), (1, 20, 27, True, 1024), (2, 100, 9, True, 1024),
                                           (1, 61, 27, False, 1024), (2, 61, 27, True, 1)])
def test_lift_equals_forward_of_the_windows_bit_for_bit(P, N, s, flip, mw, cd):
    """The whole call against its parts, with no tolerance: the demo's windows restated in numpy (resampled tail, flip_data of a copy), one
    model forward of that stacked batch, and the torch restatement of the merge and scatter.  Covers the resampled, mirrored tail whatever the
    model's conditioning, in both modes, and the chunked path (max_windows=1: per-window forwards equal the stacked one, see below)."""
    import kasportsformer_amd as K
    m = _model(cd)
    kp = _track(P, N, seed=17 + N)
    got = K.lift_track(m, kp, W_PX, H_PX, stride=s, flip=flip, max_windows=mw)
    with torch.no_grad():
        pred = m(torch.from_numpy(_windows_np(kp, 27, s, flip)).cuda())
    want = _stitch_t(pred.cpu(), P, N, 27, s, flip)
    assert tuple(got.shape) == (P, N, 17, 3) and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("P,N,s", [(1, 61, 27), (2, 100, 9), (3, 20, 27)])
def test_chunked_forward_equals_one_batch(P, N, s):
    """max_windows=1 / 2 (one or two windows and their mirrors per forward) against the default single stacked batch, fp32: bit-equal, because an
    eval-mode forward computes every clip alone (BatchNorm on running statistics, no reduction across clips; also observed in bf16)."""
    import kasportsformer_amd as K
    kp = _track(P, N, seed=3)
    a = K.lift_track(_model("fp32"), kp, W_PX, H_PX, stride=s)
    b = K.lift_track(_model("fp32"), kp, W_PX, H_PX, stride=s, max_windows=1)
    c = K.lift_track(_model("fp32"), kp, W_PX, H_PX, stride=s, max_windows=2)
    assert torch.equal(b, a) and torch.equal(c, a)


def test_no_flip_is_one_forward_with_root_zeroed():
    import kasportsformer_amd as K
    m = _model("fp32")
    kp = _track(1, 27, seed=5)
    got = K.lift_track(m, kp, W_PX, H_PX, flip=False)
    x = torch.from_numpy(_windows_np(kp, 27, 27, False)).cuda()
    with torch.no_grad():
        want = m(x)
    want[:, :, 0, :] = 0
    assert tuple(got.shape) == (1, 27, 17, 3) and torch.equal(got[0], want[0])


def test_input_mode_and_autograd_contract():
    import kasportsformer_amd as K
    m = make_pair(1, 27, "fp32")[1]
    kp = _track(2, 40, seed=9)
    kp_copy = kp.copy()
    kp_dev = torch.from_numpy(kp).cuda()
    bufs = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    out = K.lift_track(m, kp, W_PX, H_PX)
    assert m.training, "the caller's training flag is restored"
    assert not out.requires_grad and out.grad_fn is None
    assert np.array_equal(kp, kp_copy)
    out_dev = K.lift_track(m, kp_dev, W_PX, H_PX)
    assert torch.equal(kp_dev.cpu(), torch.from_numpy(kp_copy)) and torch.equal(out_dev, out)
    for k, v in m.state_dict().items():                     # eval mode: no BatchNorm running-statistics update
        assert torch.equal(v, bufs[k]), k
    m.eval()
    K.lift_track(m, kp[0], W_PX, H_PX)
    assert not m.training
    assert tuple(K.lift_track(m, kp[0], W_PX, H_PX).shape) == (40, 17, 3)
    # N = 0 and P = 0: empty results of the leading shape
    e = K.lift_track(m, np.zeros((0, 17, 3), np.float32), W_PX, H_PX)
    assert e.is_cuda and tuple(e.shape) == (0, 17, 3)
    assert tuple(K.lift_track(m, np.zeros((2, 0, 17, 3), np.float32), W_PX, H_PX).shape) == (2, 0, 17, 3)
    with pytest.raises(ValueError):
        K.lift_track(m, np.zeros((5, 17, 2), np.float32), W_PX, H_PX)
    with pytest.raises(ValueError):
        K.lift_track(m, np.zeros((1, 1, 5, 17, 3), np.float32), W_PX, H_PX)
    with pytest.raises(TypeError):
        K.lift_track(m, np.zeros((5, 17, 3), np.float64), W_PX, H_PX)
    with pytest.raises(ValueError):
        K.lift_track(m, kp, W_PX, H_PX, stride=28)
    with pytest.raises(RuntimeError):
        K.lift_track(make_pair(1, 27, "fp32")[1].cpu(), kp, W_PX, H_PX)


def test_cli_writes_what_lift_track_returns(tmp_path):
    """One fresh child process: yaml + checkpoint_save checkpoint + keypoints2d.pkl -> .npy, bit for bit lift_track's output."""
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
    kp = _track(2, 61, seed=11)
    (tmp_path / "keypoints2d.pkl").write_bytes(pickle.dumps(kp))
    cmd = [sys.executable, "-m", "kasportsformer_amd.lift", "--config", str(tmp_path / "m.yaml"), "--checkpoint", str(tmp_path / "best.pth"),
           "--keypoints", str(tmp_path / "keypoints2d.pkl"), "--width", str(W_PX), "--height", str(H_PX), "--compute-dtype", "fp32", "--stride", "9",
           "--out", str(tmp_path / "poses3d.npy")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(tmp_path / "poses3d.npy")
    want = K.lift_track(m, kp, W_PX, H_PX, stride=9).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (2, 61, 17, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
