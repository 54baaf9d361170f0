"""The camera-space placement on the GPU (kasportsformer_amd.place_poses, csrc/k_place.hip): the public function and the C entry on the device equal the fp64
numpy restatement of include/kasf.h's rule (tests/place_ref.py) bit for bit on all five outputs -- at 1, 129 and 300 frames, as [N,17,3] and [2,3,17,3], with
the camera and the table as one row and per frame --, the same bits on a second run, a frame alone against the frame inside the batch, inputs unchanged,
sentinels behind the outputs intact, host and device inputs, every state seen, the NaN frames filled by refine_tracks, and the command line's --place against
the Python calls.  A differing bit is a finding to explain, not a bar to loosen."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import ptr, stream
from tests.place_ref import bundle, place_np, project, scene

pytestmark = pytest.mark.gpu
FIELDS = ("poses", "root", "residual", "scale", "state")
CAN = 9.0


def raw(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def same(result, want, shape=None):
    for name in FIELDS:
        got, ref = getattr(result, name), want[name]
        if shape is not None:
            ref = ref.reshape(shape + ref.shape[1:])
        assert tuple(got.shape) == ref.shape and got.is_cuda and got.dtype == (torch.uint8 if name == "state" else torch.float32), name
        diff = np.argwhere(raw(got).reshape(-1) != raw(ref).reshape(-1))
        assert diff.size == 0, (name, diff[:8])


@pytest.fixture(scope="module")
def cases():
    """The inputs and the restatement's outputs of the tests here, made once: (frames, per_frame) -> (P, K, camera, lengths, want)."""
    out = {}
    for frames, per_frame in ((1, False), (129, False), (129, True), (300, False), (300, True)):
        P, K, camera, lengths = bundle(frames, seed=frames, per_frame=per_frame)
        out[frames, per_frame] = (P, K, camera, lengths, place_np(P, K, camera, lengths))
    return out


@pytest.mark.parametrize("frames,per_frame", [(1, False), (129, False), (129, True), (300, False), (300, True)])
def test_place_poses_equals_the_restatement_bit_for_bit(cases, frames, per_frame):
    import kasportsformer_amd as K_
    P, K, camera, lengths, want = cases[frames, per_frame]
    Pd, Kd = torch.from_numpy(P).cuda(), torch.from_numpy(K).cuda()
    r = K_.place_poses(Pd, Kd, camera, metric_lengths=lengths)
    assert isinstance(r, K_.PlaceResult)
    same(r, want)
    same(K_.place_poses(Pd, Kd, torch.from_numpy(camera).cuda(), metric_lengths=torch.from_numpy(lengths).cuda()), want)      # the same bits on a second run
    same(K_.place_poses(P, K, camera, metric_lengths=lengths), want)                                                         # from the host
    assert np.array_equal(raw(Pd), raw(P)) and np.array_equal(raw(Kd), raw(K))
    if frames >= 129:
        assert set(np.unique(want["state"]).tolist()) == {0, 1, 2, 3}                                                        # every state seen


def test_without_a_table_and_other_parameters():
    import kasportsformer_amd as K_
    P, K, camera, _ = bundle(300, seed=3, table=False, per_frame=True)
    for q in (dict(iterations=0), dict(iterations=1, weighted=False), dict(iterations=8, delta=1.5, min_joints=9, min_score=0.5)):
        want = place_np(P, K, camera, None, **q)
        same(K_.place_poses(P, K, camera, **q), want)
    assert set(np.unique(want["state"]).tolist()) >= {0, 1, 2}


def test_leading_shapes(cases):
    import kasportsformer_amd as K_
    P, K, camera, lengths, want = cases[300, True]
    P6, K6, c6, l6 = P[:6].reshape(2, 3, 17, 3), K[:6].reshape(2, 3, 17, 3), camera[:6].reshape(2, 3, 4), lengths[:6].reshape(2, 3, 16)
    same(K_.place_poses(P6, K6, c6, metric_lengths=l6), {k: v[:6] for k, v in want.items()}, (2, 3))
    one = K_.place_poses(P[0], K[0], camera[0], metric_lengths=lengths[0])                                                   # a single frame [17,3]
    assert one.poses.shape == (17, 3) and one.root.shape == (3,) and one.state.shape == ()
    assert np.array_equal(raw(one.poses), raw(want["poses"][0])) and np.array_equal(raw(one.root), raw(want["root"][0]))
    empty = K_.place_poses(P[:0], K[:0], camera[0])
    assert empty.poses.shape == (0, 17, 3) and empty.state.shape == (0,) and empty.root.is_cuda


def test_a_frame_alone_equals_the_frame_in_the_batch(cases):
    import kasportsformer_amd as K_
    P, K, camera, lengths, want = cases[129, True]
    full = K_.place_poses(P, K, camera, metric_lengths=lengths)
    for f in (0, 63, 64, 128):
        one = K_.place_poses(P[f:f + 1], K[f:f + 1], camera[f:f + 1], metric_lengths=lengths[f:f + 1])
        for name in FIELDS:
            assert np.array_equal(raw(getattr(one, name)), raw(getattr(full, name)[f:f + 1])), (f, name)


@pytest.mark.parametrize("offset", [0, 1])
def test_the_entry_writes_nothing_else_and_takes_null_outputs(cases, offset):
    """The C entry with sentinels around every output, at 16-byte aligned pointers and at pointers 4 bytes past them; then each optional output NULL in turn."""
    from kasportsformer_amd import _lib
    P, K, camera, lengths, want = cases[300, False]
    N = len(P)
    lib = _lib.load()

    def at(a):                                                          # a device copy `offset` floats past a 16-byte boundary
        buf = torch.zeros(a.size + 8, device="cuda")
        buf[offset:offset + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        return buf[offset:offset + a.size]

    Pd, Kd, cd, ld = at(P), at(K), torch.from_numpy(camera).cuda(), torch.from_numpy(lengths).cuda()
    q = _lib.KasfPlaceParams(0.3, 1, 4, 3.0, 4)
    sizes = {"poses": N * 51, "root": N * 3, "residual": N, "scale": N, "state": N}
    for null in (None, "root", "residual", "scale", "state"):
        bufs = {k: torch.full((n + 128 + offset,), 77 if k == "state" else CAN, dtype=torch.uint8 if k == "state" else torch.float32, device="cuda")
                for k, n in sizes.items()}
        lo = {k: 64 + (offset if k == "poses" else 0) for k in sizes}
        view = {k: bufs[k][lo[k]:lo[k] + n] for k, n in sizes.items()}
        arg = lambda k: None if k == null else ptr(view[k])             # noqa: E731
        _lib.check(lib.kasf_pose_place(ptr(Pd), ptr(Kd), N, ptr(cd), 0, ptr(ld), 0, C.byref(q), arg("poses"), arg("root"), arg("residual"), arg("scale"),
                                       arg("state"), stream()))
        for k, n in sizes.items():
            fill = 77 if k == "state" else CAN
            assert (bufs[k][:lo[k]] == fill).all() and (bufs[k][lo[k] + n:] == fill).all(), (null, k)
            if k == null:
                assert (view[k] == fill).all()
            else:
                assert np.array_equal(raw(view[k]), raw(want[k]).reshape(-1) if k == "state" else raw(want[k].reshape(-1))), (null, k)
    assert np.array_equal(raw(Pd), raw(P.reshape(-1))) and np.array_equal(raw(Kd), raw(K.reshape(-1)))
    assert np.array_equal(raw(cd), raw(camera)) and np.array_equal(raw(ld), raw(lengths))


def test_frames_that_are_not_placed_are_filled_by_refine_tracks():
    import kasportsformer_amd as K_
    n = 120
    P, _, _, camera = scene(np.random.default_rng(8), n)
    t = np.linspace(0.0, 1.0, n)
    T = np.stack([-3.0 + 6.0 * t, 0.5 * np.ones(n), 10.0 + 8.0 * t], 1)
    K = np.concatenate([project(P.astype(np.float64) + T[:, None, :], camera), np.full((n, 17, 1), 0.9)], -1).astype(np.float32)
    lost = (np.arange(n) % 17 == 5) | ((np.arange(n) >= 60) & (np.arange(n) < 66))
    K[lost, :, 2] = 0.0
    r = K_.place_poses(P, K, camera)
    assert np.array_equal(r.state.cpu().numpy() != 0, lost) and torch.isnan(r.root[torch.from_numpy(lost).cuda()]).all()
    root, st = K_.refine_tracks(r.root.unsqueeze(-2), score=False, return_state=True)
    assert np.array_equal(st[:, 0].cpu().numpy() == 1, lost) and torch.isfinite(root).all()
    assert np.abs(root[:, 0].cpu().numpy().astype(np.float64) - T).max() < 1e-3
    world = K_.poses_to_world(r.poses)                                   # the chain composes: placed poses go on to world space
    assert world.shape == r.poses.shape


def test_cli_place_writes_what_the_python_calls_give(tmp_path):
    """``--place`` in process, on a one-layer model: an .npz of two tracks gets the placed poses, root_i and place_state_i; an .npy the placed poses only;
    --place runs before --world."""
    import yaml
    import kasportsformer_amd as K_
    from kasportsformer_amd.lift import main
    from tests.gpu_util import make_pair
    from tests.place_ref import BONES_170
    m = make_pair(1, 27, "fp32")[1].eval()
    cfg = {"model_name": "KASportsFormer", "n_layers": 1, "dim_in": 3, "dim_feat": 128, "dim_rep": 512, "dim_out": 3, "mlp_ratio": 4, "act_layer": "gelu",
           "attn_drop": 0.0, "drop": 0.0, "drop_path": 0.0, "use_layer_scale": True, "layer_scale_init_value": 0.00001, "use_adaptive_fusion": True,
           "num_heads": 8, "qkv_bias": False, "qkv_scale": None, "hierarchical": False, "num_joints": 17, "use_temporal_similarity": True,
           "neighbour_num": 4, "temporal_connection_len": 1, "use_tcn": False, "graph_only": False, "n_frames": 27}
    (tmp_path / "m.yaml").write_text(yaml.safe_dump(cfg))
    K_.checkpoint_save(str(tmp_path / "best.pth"), 0, 1e-3, None, m, 100.0, "x")
    rng = np.random.default_rng(12)
    tracks = [scene(rng, n, size=(1280.0, 720.0))[2] for n in (40, 31)]
    np.savez(tmp_path / "tracks.npz", *tracks)
    np.save(tmp_path / "one.npy", tracks[0])
    np.save(tmp_path / "table.npy", BONES_170)
    camera = np.array([1500, 1500, 640, 360], np.float32)
    base = ["--config", str(tmp_path / "m.yaml"), "--checkpoint", str(tmp_path / "best.pth"), "--width", "1280", "--height", "720", "--compute-dtype", "fp32",
            "--place", "--camera", "1500,1500,640,360"]
    lifted = K_.lift_tracks(m, tracks, 1280, 720)
    main(base + ["--keypoints", str(tmp_path / "tracks.npz"), "--out", str(tmp_path / "out.npz"), "--place-lengths", str(tmp_path / "table.npy"),
                 "--place-iterations", "2", "--place-delta", "4.0"])
    with np.load(tmp_path / "out.npz") as z:
        assert sorted(z.files) == ["place_state_0", "place_state_1", "root_0", "root_1", "track_0", "track_1"]
        for i, (kp, pose) in enumerate(zip(tracks, lifted)):
            want = K_.place_poses(pose, kp, camera, metric_lengths=BONES_170, iterations=2, delta=4.0)
            assert np.array_equal(raw(z[f"track_{i}"]), raw(want.poses)) and np.array_equal(raw(z[f"root_{i}"]), raw(want.root))
            assert np.array_equal(z[f"place_state_{i}"], want.state.cpu().numpy()) and z[f"place_state_{i}"].dtype == np.uint8
    main(base + ["--keypoints", str(tmp_path / "one.npy"), "--out", str(tmp_path / "one_out.npy"), "--world", "--world-floor"])
    want = K_.poses_to_world(K_.place_poses(K_.lift_track(m, tracks[0], 1280, 720), tracks[0], camera).poses, floor=True)
    assert np.array_equal(raw(np.load(tmp_path / "one_out.npy")), raw(want))
