"""Host side of the lift's two ends (kasportsformer_amd.coco_to_h36m / poses_to_world, kasf_coco_h36m / kasf_pose_world): the fixture written by the
real reference helpers (tests/golden/make_coco_golden.py), the sequential-fp32 restatements the GPU tests hold the kernels to (tests/test_gpu_coco_world.py
imports them from here) tied to that fixture, the refusals of the two entry points and of the Python surface, and the command line."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32


def fixture():
    return np.load(os.path.join(GOLDEN, "coco_world.npz"), allow_pickle=False)


def coco_h36m_np(coco):
    """h36m_coco_format (demo/lib/preprocess.py:10-69) on [...,17,3] float32 COCO x, y, score, restated statement by statement in sequential fp32:
    left-to-right sums, a divide by the count, no fused multiply-add.  Shapes are kept (no all-zero person is dropped)."""
    k = np.ascontiguousarray(coco, dtype=F32)
    h = np.zeros_like(k)
    two, three, four = F32(2), F32(3), F32(4)
    h[..., [9, 11, 14, 12, 15, 13, 16, 4, 1, 5, 2, 6, 3], :] = k[..., [0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16], :]
    xy, nose = k[..., :2], k[..., 0, :2]
    shoulders = (xy[..., 5, :] + xy[..., 6, :]) / two
    h[..., 10, 0] = (((k[..., 1, 0] + k[..., 2, 0]) + k[..., 3, 0]) + k[..., 4, 0]) / four                   # :16 head
    h[..., 10, 1] = (k[..., 1, 1] + k[..., 2, 1]) - k[..., 0, 1]                                             # :17
    h[..., 8, :2] = shoulders + (nose - shoulders) / three                                                   # :18-19 thorax
    h[..., 0, :2] = (xy[..., 11, :] + xy[..., 12, :]) / two                                                  # :21 pelvis
    h[..., 7, :2] = (((xy[..., 5, :] + xy[..., 6, :]) + xy[..., 11, :]) + xy[..., 12, :]) / four             # :22 spine
    h[..., 9, :2] = nose - (nose - shoulders) / four                                                         # :27 neck: the copied nose
    h[..., 7, 0] = h[..., 7, 0] + two * (h[..., 7, 0] - (h[..., 0, 0] + h[..., 8, 0]) / two)                 # :28 spine x
    h[..., 8, 1] = h[..., 8, 1] - (((k[..., 1, 1] + k[..., 2, 1]) / two - k[..., 0, 1]) * two) / three       # :29 thorax y, after :28
    s = k[..., 2]
    h[..., 0, 2] = (s[..., 11] + s[..., 12]) / two                                                           # :59-62
    h[..., 8, 2] = (s[..., 5] + s[..., 6]) / two
    h[..., 7, 2] = (h[..., 0, 2] + h[..., 8, 2]) / two
    h[..., 10, 2] = (((s[..., 1] + s[..., 2]) + s[..., 3]) + s[..., 4]) / four
    assert h.dtype == F32
    return h


def world_np(poses, rot, t=(0.0, 0.0, 0.0), floor=False, unit=False):
    """camera_to_world (qrot, demo/lib/utils.py:55-73) plus t, then demo.py:246 (floor) and :247-248 (unit), in sequential fp32: every product and sum
    its own rounding, torch.cross's component order, v + 2 * (q0 * uv + uuv)."""
    v = np.ascontiguousarray(poses, dtype=F32)
    q0, q1, q2, q3 = (F32(a) for a in rot)
    t0, t1, t2 = (F32(a) for a in t)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    ux, uy, uz = q2 * z - q3 * y, q3 * x - q1 * z, q1 * y - q2 * x
    wx, wy, wz = q2 * uz - q3 * uy, q3 * ux - q1 * uz, q1 * uy - q2 * ux
    out = np.stack(((x + F32(2) * (q0 * ux + wx)) + t0, (y + F32(2) * (q0 * uy + wy)) + t1, (z + F32(2) * (q0 * uz + wz)) + t2), axis=-1)
    if floor:
        out[..., 2] = out[..., 2] - out[..., 2].min(axis=-1, keepdims=True)
    if unit:
        out = out / out.max(axis=(-2, -1), keepdims=True)
    assert out.dtype == F32
    return out


def world_f64(poses, rot, t=(0.0, 0.0, 0.0), floor=False, unit=False):
    """The same formula evaluated in float64 on the float32 inputs."""
    v, q, t = np.asarray(poses, np.float64), np.asarray(rot, F32).astype(np.float64), np.asarray(t, F32).astype(np.float64)
    qv = np.broadcast_to(q[1:], v.shape)
    uv = np.cross(qv, v)
    out = v + 2 * (q[0] * uv + np.cross(qv, uv)) + t
    if floor:
        out[..., 2] -= out[..., 2].min(axis=-1, keepdims=True)
    if unit:
        out /= out.max(axis=(-2, -1), keepdims=True)
    return out


def test_fixture_loads_without_pickles_and_is_small():
    path = os.path.join(GOLDEN, "coco_world.npz")
    assert os.path.getsize(path) < 200 * 1024
    fx = fixture()
    coco = fx["coco"]
    P, N = coco.shape[:2]
    assert coco.dtype == F32 and coco.shape == (P, N, 17, 3) and P >= 3 and N >= 61
    assert fx["h36m_kpts"].shape == (P, N, 17, 2) and fx["h36m_scores"].shape == (P, N, 17)
    zero = [(p, f) for p in range(P) for f in range(N) if not coco[p, f].any()]
    assert len(zero) == 1 and coco[zero[0][0]].any(), "one all-zero frame inside a non-zero track"
    xy = coco[..., :2]
    assert xy.max() > 3000 and xy.max() <= 4000 and xy.min() >= 0 and ((xy > 0) & (xy < 1)).sum() > 100, "0-4,000 px, some sub-pixel"
    lifts = np.load(os.path.join(GOLDEN, "lift_e2e.npz"), allow_pickle=False)
    for name in ("lift_n61", "lift_p2"):
        assert fx["post_" + name].shape == fx["c2w_" + name].shape == lifts[name].shape and fx["post_" + name].dtype == F32
    assert fx["rot"].shape == (4,) and fx["t"].shape == (3,) and fx["t"].any()
    assert 0 < float(fx["world_err_ref"]) < 1e-6


def test_restated_conversion_is_the_reference_bit_for_bit():
    fx = fixture()
    got = coco_h36m_np(fx["coco"])
    assert np.array_equal(got[..., :2], fx["h36m_kpts"])
    assert np.array_equal(got[..., 2], fx["h36m_scores"])
    p, f = next((p, f) for p in range(fx["coco"].shape[0]) for f in range(fx["coco"].shape[1]) if not fx["coco"][p, f].any())
    assert not got[p, f].any(), "an all-zero frame converts to an all-zero frame"


def test_restated_world_step_is_within_twice_the_reference_error():
    """Reference and restatement are both fp32 roundings of one formula; the reference's own largest deviation from the float64 evaluation
    (world_err_ref, computed by the generator) times 2 covers a different but equally valid rounding order."""
    fx = fixture()
    lifts = np.load(os.path.join(GOLDEN, "lift_e2e.npz"), allow_pickle=False)
    ref_err, worst = float(fx["world_err_ref"]), 0.0
    for name in ("lift_n61", "lift_p2"):
        x = lifts[name]
        for tag, kw in (("post_", dict(floor=True, unit=True)), ("c2w_", dict(t=fx["t"]))):
            mine, exact = world_np(x, fx["rot"], **kw), world_f64(x, fx["rot"], **kw)
            err = float(np.abs(mine - exact).max())
            print(f"{tag}{name}: restatement vs float64 {err:.3e} = {err / ref_err:.3f} x world_err_ref ({ref_err:.3e}); "
                  f"restatement vs reference {float(np.abs(mine - fx[tag + name]).max()):.3e}")
            worst = max(worst, err)
    assert worst <= 2 * ref_err, (worst, ref_err)


def test_entry_points_refuse_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    buf = np.zeros(51, F32)
    p, q = buf.ctypes.data_as(C.c_void_p), np.zeros(4, F32).ctypes.data_as(C.c_void_p)
    coco = lib.kasf_coco_h36m                                   # (coco, frames, h36m, stream)
    assert coco(None, 0, None, None) == 0                       # nothing to do
    assert coco(p, -1, p, None) == 2 and lib.kasf_last_error()
    assert coco(None, 1, p, None) == 2
    assert coco(p, 1, None, None) == 2
    world = lib.kasf_pose_world                                 # (poses, frames, quat4, trans3, floor, unit, out, stream)
    assert world(None, 0, None, None, 1, 1, None, None) == 0
    assert world(p, -1, q, None, 0, 0, p, None) == 2
    assert world(None, 1, q, None, 0, 0, p, None) == 2
    assert world(p, 1, None, None, 0, 0, p, None) == 2          # the rotation is required, the translation is not
    assert world(p, 1, q, None, 0, 0, None, None) == 2
    assert lib.kasf_last_error()
    assert not buf.any()


def test_python_surface_has_no_host_path():
    import kasportsformer_amd as K
    coco = np.zeros((4, 17, 3), F32)
    with pytest.raises(RuntimeError):
        K.coco_to_h36m(coco, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            K.coco_to_h36m(coco)
        with pytest.raises(RuntimeError):
            K.coco_to_h36m(torch.zeros((2, 4, 17, 2)), torch.zeros((2, 4, 17)))
    with pytest.raises(RuntimeError):
        K.poses_to_world(torch.zeros((4, 17, 3)))
    for exc, call in ((TypeError, lambda: K.coco_to_h36m(coco.astype(np.float64))),
                      (TypeError, lambda: K.coco_to_h36m(coco.tolist())),
                      (ValueError, lambda: K.coco_to_h36m(coco[:, :, :2])),
                      (ValueError, lambda: K.coco_to_h36m(coco[:, :, :2], coco[:, :5, 2])),
                      (ValueError, lambda: K.coco_to_h36m(coco, coco[..., 2])),
                      (TypeError, lambda: K.poses_to_world(coco)),
                      (TypeError, lambda: K.poses_to_world(torch.zeros((4, 17, 3), dtype=torch.float64)))):
        with pytest.raises(exc):
            call()
    assert len(K.DEMO_CAMERA_ROTATION) == 4 and abs(sum(a * a for a in K.DEMO_CAMERA_ROTATION) - 1) < 1e-6
    assert np.array_equal(np.asarray(K.DEMO_CAMERA_ROTATION, F32), fixture()["rot"])
    assert not coco.any()


def test_a_bad_layout_raises_from_all_three_lift_surfaces():
    import kasportsformer_amd as K
    m = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=27, compute_dtype="fp32")
    kp = np.zeros((5, 17, 3), F32)
    for bad in ("COCO", "coco17", None, 0):
        with pytest.raises(ValueError, match="layout"):
            K.lift_track(m, kp, 1280, 720, layout=bad)
        with pytest.raises(ValueError, match="layout"):
            K.lift_tracks(m, [kp], 1280, 720, layout=bad)
        with pytest.raises(ValueError, match="layout"):
            K.lift_tracks(m, kp, 1280, 720, offsets=[0, 5], layout=bad)
        with pytest.raises(ValueError, match="layout"):
            K.StreamLifter(m, 1280, 720, slots=2, layout=bad)
    for good in ("h36m", "coco"):                               # a known layout gets as far as the missing GPU
        with pytest.raises(RuntimeError):
            K.lift_track(m, kp, 1280, 720, layout=good)
        with pytest.raises(RuntimeError):
            K.StreamLifter(m, 1280, 720, slots=2, layout=good)


def test_abi_version_is_at_least_11():
    from kasportsformer_amd import _lib
    assert _lib.ABI_VERSION == _lib.load().kasf_version() >= 11       # the two entries are ABI 11's; tests/test_cabi_cpu.py pins the current number
    assert "kasf_coco_h36m" in _lib.SIGNATURES and "kasf_pose_world" in _lib.SIGNATURES


def test_cli_parser_accepts_the_new_options(capsys):
    from kasportsformer_amd.lift import _parse
    base = ["--config", "m.yaml", "--checkpoint", "best.pth", "--keypoints", "kp.pkl", "--width", "1280", "--height", "720", "--out", "o.npy"]
    a = _parse(base + ["--layout", "coco", "--world"])
    assert a.layout == "coco" and a.world and not a.world_floor and not a.world_unit
    a = _parse(base + ["--layout", "coco", "--world", "--world-floor", "--world-unit", "--online", "--lag", "3"])
    assert a.world_floor and a.world_unit and a.online and a.lag == 3
    a = _parse(base)
    assert a.layout == "h36m" and not a.world
    for bad in (["--layout", "openpose"], ["--world-floor"], ["--world-unit"]):
        with pytest.raises(SystemExit):
            _parse(base + bad)
    capsys.readouterr()
