"""The lift's two ends on the GPU (kasportsformer_amd.coco_to_h36m / poses_to_world, kasf_coco_h36m / kasf_pose_world, ``layout="coco"``): the conversion
bit for bit against the reference's own output (tests/golden/coco_world.npz) and against the restatement tied to it on the CPU
(tests/test_coco_world_cpu.py), the world step bit for bit against that file's sequential-fp32 restatement, ``layout="coco"`` on the three lift surfaces
against converting first, the default layout against its explicit spelling, and the CLI."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.test_coco_world_cpu import GOLDEN, coco_h36m_np, fixture, world_f64, world_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_PX, H_PX = 1280, 720
_MODELS = {}


def _model(cd):
    if cd not in _MODELS:
        _MODELS[cd] = make_pair(2, 27, cd)[1].eval()
    return _MODELS[cd]


def _coco(shape, seed, size=4000.0):
    """COCO-17 x, y, score of ``shape`` frames: pixels up to ``size`` with every joint scaled by 1, 0.1, 0.01 or 0.001, scores in [0, 1]."""
    g = np.random.default_rng(seed)
    shape = tuple(np.atleast_1d(shape))
    xy = g.uniform(0, size, size=shape + (17, 2)) * 10.0 ** g.integers(-3, 1, size=shape + (17, 1))
    return np.concatenate((xy, g.uniform(0, 1, size=shape + (17, 1))), axis=-1).astype(np.float32)


def test_conversion_is_the_reference_bit_for_bit():
    import kasportsformer_amd as K
    fx = fixture()
    coco = fx["coco"]
    keep = coco.copy()
    want = torch.from_numpy(np.concatenate((fx["h36m_kpts"], fx["h36m_scores"][..., None]), axis=-1))
    xy, sc = np.ascontiguousarray(coco[..., :2]), np.ascontiguousarray(coco[..., 2])
    on_dev = torch.from_numpy(coco).cuda()
    xy_d, sc_d = torch.from_numpy(xy).cuda(), torch.from_numpy(sc).cuda()
    for got in (K.coco_to_h36m(coco), K.coco_to_h36m(torch.from_numpy(coco)), K.coco_to_h36m(on_dev), K.coco_to_h36m(coco, device="cuda:0"),
                K.coco_to_h36m(xy, sc), K.coco_to_h36m(torch.from_numpy(xy), torch.from_numpy(sc)), K.coco_to_h36m(xy_d, sc_d), K.coco_to_h36m(xy, sc_d)):
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == coco.shape and not got.requires_grad
        assert torch.equal(got.cpu(), want)
    assert np.array_equal(coco, keep) and np.array_equal(xy, keep[..., :2]) and np.array_equal(sc, keep[..., 2])
    assert torch.equal(on_dev.cpu(), torch.from_numpy(keep)) and torch.equal(xy_d.cpu(), torch.from_numpy(xy)) and torch.equal(sc_d.cpu(), torch.from_numpy(sc))
    one = K.coco_to_h36m(coco[1, 30])                                   # a single frame, the all-zero one
    assert tuple(one.shape) == (17, 3) and not one.any()
    with pytest.raises(RuntimeError):
        K.coco_to_h36m(on_dev, device="cpu")


def test_conversion_of_20000_frames_and_of_none():
    import kasportsformer_amd as K
    from kasportsformer_amd import _lib
    coco = _coco(20000, seed=1)
    coco[123] = 0
    want = torch.from_numpy(coco_h36m_np(coco))
    dev = torch.from_numpy(coco).cuda()
    assert torch.equal(K.coco_to_h36m(dev).cpu(), want)
    assert torch.equal(K.coco_to_h36m(coco.reshape(4, 50, 100, 17, 3)).cpu(), want.view(4, 50, 100, 17, 3))
    # a view that starts at frame 1 is not 16-byte aligned: the one-float-per-lane form of the kernel, and a last tile that is not full
    assert dev[1:].data_ptr() % 16 != 0
    assert torch.equal(K.coco_to_h36m(dev[1:]).cpu(), want[1:])
    for n in (1, 127, 128, 129):
        assert torch.equal(K.coco_to_h36m(dev[:n]).cpu(), want[:n]), n
    assert torch.equal(dev.cpu(), torch.from_numpy(coco))
    empty = K.coco_to_h36m(np.zeros((0, 17, 3), np.float32))
    assert empty.is_cuda and tuple(empty.shape) == (0, 17, 3)
    assert tuple(K.coco_to_h36m(np.zeros((3, 0, 17, 2), np.float32), np.zeros((3, 0, 17), np.float32)).shape) == (3, 0, 17, 3)
    out = torch.full((4, 17, 3), 7.0, device="cuda")
    _lib.check(_lib.load().kasf_coco_h36m(ptr(dev), 0, ptr(out), stream()))
    torch.cuda.synchronize()
    assert (out == 7).all(), "frames = 0 writes nothing"


WORLD_CASES = [("rotation only", dict()), ("rotation + t", dict(t=(0.25, -0.5, 1.0))), ("floor", dict(floor=True)), ("floor + unit", dict(floor=True, unit=True)),
               ("unit", dict(unit=True)), ("t + floor + unit", dict(t=(3.0, 0.125, -2.0), floor=True, unit=True))]


@pytest.mark.parametrize("name,kw", WORLD_CASES, ids=[c[0] for c in WORLD_CASES])
def test_world_step_equals_the_fp32_restatement(name, kw):
    """torch.equal against tests/test_coco_world_cpu.py's world_np, which that file ties to the reference; on the fixture's inputs also within twice
    the reference's own error of the float64 evaluation, as the restatement is."""
    import kasportsformer_amd as K
    fx = fixture()
    lifts = np.load(os.path.join(GOLDEN, "lift_e2e.npz"), allow_pickle=False)
    call = dict(floor=kw.get("floor", False), unit=kw.get("unit", False))
    if "t" in kw:
        call["translation"] = kw["t"]
    g = np.random.default_rng(5)
    big = (g.standard_normal((5000, 17, 3)) * 10.0 ** g.integers(-2, 2, size=(5000, 1, 1))).astype(np.float32)
    big[:, 0] = 0
    for tag, x in (("lift_n61", lifts["lift_n61"]), ("lift_p2", lifts["lift_p2"]), ("random", big), ("one", big[7]), ("odd", big[1:400])):
        x = np.ascontiguousarray(x)
        dev = torch.from_numpy(big).cuda()[1:400] if tag == "odd" else torch.from_numpy(x).cuda()      # "odd": not 16-byte aligned, a partial last tile
        assert (dev.data_ptr() % 16 != 0) == (tag == "odd")
        got = K.poses_to_world(dev, rotation=fx["rot"], **call)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == x.shape and got.data_ptr() != dev.data_ptr()
        assert torch.equal(got.cpu(), torch.from_numpy(world_np(x, fx["rot"], **kw))), (name, tag)
        assert torch.equal(dev.cpu(), torch.from_numpy(x))
        if tag.startswith("lift_"):
            err = float(np.abs(got.cpu().numpy() - world_f64(x, fx["rot"], **kw)).max())
            print(f"{name} / {tag}: kernel vs float64 {err:.3e} = {err / float(fx['world_err_ref']):.3f} x world_err_ref")
            if name in ("rotation + t", "floor + unit"):              # the two results of the reference that world_err_ref was taken over
                assert err <= 2 * float(fx["world_err_ref"]), (name, tag, err)
    if "t" not in kw:                                                 # the default rotation is the demo's
        p2 = lifts["lift_p2"]
        assert torch.equal(K.poses_to_world(torch.from_numpy(p2).cuda(), **call).cpu(), torch.from_numpy(world_np(p2, K.DEMO_CAMERA_ROTATION, **kw)))


def test_world_step_edges():
    import kasportsformer_amd as K
    from kasportsformer_amd import _lib
    fx = fixture()
    empty = K.poses_to_world(torch.zeros((2, 0, 17, 3), device="cuda"), floor=True, unit=True)
    assert empty.is_cuda and tuple(empty.shape) == (2, 0, 17, 3)
    # a frame whose largest value is 0 gets the reference's division: 0 / 0
    x = np.zeros((3, 17, 3), np.float32)
    x[1] = np.random.default_rng(0).standard_normal((17, 3)).astype(np.float32)
    got = K.poses_to_world(torch.from_numpy(x).cuda(), floor=True, unit=True).cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = world_np(x, K.DEMO_CAMERA_ROTATION, floor=True, unit=True)
    assert np.isnan(want[0]).all() and np.isnan(got[0]).all() and np.isnan(got[2]).all() and np.array_equal(got[1], want[1])
    # a non-contiguous view is read, not written
    base = torch.randn((6, 17, 3, 2), device="cuda")
    view, keep = base[..., 0], base.clone()
    got = K.poses_to_world(view, rotation=fx["rot"], translation=fx["t"])
    assert torch.equal(got.cpu(), torch.from_numpy(world_np(view.cpu().numpy(), fx["rot"], t=fx["t"]))) and torch.equal(base, keep)
    # the C entry with a null translation is t = 0
    src, out = torch.randn((130, 17, 3), device="cuda"), torch.empty((130, 17, 3), device="cuda")
    q = np.asarray(fx["rot"], np.float32)
    _lib.check(_lib.load().kasf_pose_world(ptr(src), 130, q.ctypes.data, None, 0, 0, ptr(out), stream()))
    assert torch.equal(out.cpu(), torch.from_numpy(world_np(src.cpu().numpy(), q)))
    for bad, exc in ((dict(rotation=(1.0, 0.0, 0.0)), ValueError), (dict(translation=(1.0, 2.0)), ValueError), (dict(rotation=(float("nan"), 0, 0, 0)), ValueError)):
        with pytest.raises(exc):
            K.poses_to_world(src, **bad)
    with pytest.raises(ValueError):
        K.poses_to_world(torch.zeros((4, 17, 2), device="cuda"))


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("stride", [None, 9])
def test_lift_track_with_the_coco_layout(cd, stride):
    import kasportsformer_amd as K
    m = _model(cd)
    for shape, seed in (((2, 61), 3), ((20,), 4), ((1, 1), 5)):
        coco = _coco(shape, seed, size=W_PX)
        keep = coco.copy()
        want = K.lift_track(m, K.coco_to_h36m(coco), W_PX, H_PX, stride=stride)
        for inp in (coco, torch.from_numpy(coco).cuda()):
            got = K.lift_track(m, inp, W_PX, H_PX, stride=stride, layout="coco")
            assert got.is_cuda and tuple(got.shape) == coco.shape and torch.equal(got, want), (shape, cd, stride)
        assert np.array_equal(coco, keep)
        assert not torch.equal(want, K.lift_track(m, coco, W_PX, H_PX, stride=stride)), "the layout matters"
    assert tuple(K.lift_track(m, np.zeros((0, 17, 3), np.float32), W_PX, H_PX, layout="coco").shape) == (0, 17, 3)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_lift_tracks_with_the_coco_layout(cd):
    import kasportsformer_amd as K
    m = _model(cd)
    lengths = [33, 0, 1, 61, 27, 5]
    tracks = [_coco(n, seed=40 + i, size=W_PX) for i, n in enumerate(lengths)]
    ws, hs = [1280, 1920, 640, 3840, 1000, 1437], [720, 1080, 480, 2160, 1000, 913]
    conv = [K.coco_to_h36m(t) for t in tracks]
    for kw in (dict(), dict(max_windows=2), dict(stride=9, max_windows=3)):
        want = K.lift_tracks(m, conv, ws, hs, **kw)
        got = K.lift_tracks(m, tracks, ws, hs, layout="coco", **kw)
        assert [tuple(g.shape) for g in got] == [(n, 17, 3) for n in lengths]
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (i, kw)
        packed, off = np.concatenate(tracks), np.cumsum([0] + lengths)
        got_p = K.lift_tracks(m, torch.from_numpy(packed).cuda(), ws, hs, offsets=off, layout="coco", **kw)
        assert torch.equal(got_p, K.lift_tracks(m, K.coco_to_h36m(packed), ws, hs, offsets=off, **kw)) and torch.equal(got_p, torch.cat(want))
    assert K.lift_tracks(m, [], W_PX, H_PX, layout="coco") == []


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_stream_lifter_with_the_coco_layout(cd):
    """Two lifters tick by tick: one takes COCO frames, the other the same frames converted first.  Every slot, subsets, tail, a reset between two
    histories, replay."""
    import kasportsformer_amd as K
    m, S, lag = _model(cd), 4, 3
    a = K.StreamLifter(m, W_PX, H_PX, slots=S, lag=lag, layout="coco")
    b = K.StreamLifter(m, W_PX, H_PX, slots=S, lag=lag)
    assert a.layout == "coco" and b.layout == "h36m"
    script = [None, None, [2, 0], [3], None, [1, 3, 0]] * 6
    for tick, ids in enumerate(script):
        if tick == 20:
            a.reset(slots=[1, 2])
            b.reset(slots=[1, 2])
        k = S if ids is None else len(ids)
        coco = _coco(k, seed=300 + tick, size=W_PX)
        keep = coco.copy()
        inp = coco if tick % 2 else torch.from_numpy(coco).cuda()
        assert torch.equal(a.push(inp, slots=ids), b.push(K.coco_to_h36m(coco), slots=ids)), tick
        assert np.array_equal(coco, keep) and np.array_equal(a.counts, b.counts)
        if tick % 5 == 4:
            assert torch.equal(a.tail(), b.tail()) and torch.equal(a.tail(slots=[3, 0]), b.tail(slots=[3, 0])), tick
    assert torch.equal(a._ring, b._ring), "the ring holds H36M frames"
    assert a.counts.max() > 27 and a.counts.min() < 20
    for shape in ((40,), (2, 33), (1, 5)):
        track = _coco(shape, seed=77, size=W_PX)
        ring, counts = a._ring.clone(), a.counts
        got = a.replay(track)
        assert torch.equal(got, b.replay(K.coco_to_h36m(track))), shape
        assert not torch.equal(got, b.replay(track))
        assert torch.equal(a._ring, ring) and np.array_equal(a.counts, counts)


def test_the_default_layout_is_h36m():
    import kasportsformer_amd as K
    m = _model("fp32")
    kp = _coco((2, 40), seed=9, size=W_PX)
    assert torch.equal(K.lift_track(m, kp, W_PX, H_PX), K.lift_track(m, kp, W_PX, H_PX, layout="h36m"))
    tracks = [kp[0], kp[1, :7]]
    for g, w in zip(K.lift_tracks(m, tracks, W_PX, H_PX), K.lift_tracks(m, tracks, W_PX, H_PX, layout="h36m")):
        assert torch.equal(g, w)
    a, b = K.StreamLifter(m, W_PX, H_PX, slots=2), K.StreamLifter(m, W_PX, H_PX, slots=2, layout="h36m")
    for f in range(5):
        assert torch.equal(a.push(kp[:, f]), b.push(kp[:, f]))
    assert torch.equal(a.replay(kp), b.replay(kp))


def test_cli_with_coco_layout_and_world_output(tmp_path):
    """One fresh child process per call: --layout coco --world --world-floor --world-unit writes, bit for bit, what the Python calls give."""
    import yaml
    import kasportsformer_amd as K
    m = make_pair(1, 27, "fp32")[1].eval()
    cfg = {"model_name": "KASportsFormer", "n_layers": 1, "dim_in": 3, "dim_feat": 128, "dim_rep": 512, "dim_out": 3, "mlp_ratio": 4, "act_layer": "gelu",
           "attn_drop": 0.0, "drop": 0.0, "drop_path": 0.0, "use_layer_scale": True, "layer_scale_init_value": 0.00001, "use_adaptive_fusion": True,
           "num_heads": 8, "qkv_bias": False, "qkv_scale": None, "hierarchical": False, "num_joints": 17, "use_temporal_similarity": True,
           "neighbour_num": 4, "temporal_connection_len": 1, "use_tcn": False, "graph_only": False, "n_frames": 27}
    (tmp_path / "m.yaml").write_text(yaml.safe_dump(cfg))
    K.checkpoint_save(str(tmp_path / "best.pth"), 0, 1e-3, None, m, 100.0, "x")
    coco = _coco((2, 40), seed=11, size=W_PX)
    (tmp_path / "coco.pkl").write_bytes(pickle.dumps(coco))
    base = [sys.executable, "-m", "kasportsformer_amd.lift", "--config", str(tmp_path / "m.yaml"), "--checkpoint", str(tmp_path / "best.pth"),
            "--width", str(W_PX), "--height", str(H_PX), "--compute-dtype", "fp32", "--keypoints", str(tmp_path / "coco.pkl")]

    def run(extra, out):
        r = subprocess.run(base + extra + ["--out", str(tmp_path / out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.load(tmp_path / out)

    lift = K.lift_track(m, coco, W_PX, H_PX, layout="coco")
    for extra, want in ((["--layout", "coco", "--world", "--world-floor", "--world-unit"], K.poses_to_world(lift, floor=True, unit=True)),
                        (["--layout", "coco", "--world"], K.poses_to_world(lift)),
                        (["--layout", "coco"], lift)):
        got, want = run(extra, "poses3d.npy"), want.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (2, 40, 17, 3)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), extra
    online = K.StreamLifter(m, W_PX, H_PX, slots=1, lag=4, layout="coco").replay(coco)
    got = run(["--layout", "coco", "--world", "--world-floor", "--online", "--lag", "4"], "online.npy")
    assert np.array_equal(got.view(np.uint32), K.poses_to_world(online, floor=True).cpu().numpy().view(np.uint32))
    r = subprocess.run(base + ["--world-unit", "--out", str(tmp_path / "no.npy")], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and not (tmp_path / "no.npy").exists()
