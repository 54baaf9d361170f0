"""csrc/k_triangulate.hip without a GPU: the kernels' own source compiled for the host with g++ behind a lockstep emulation of a workgroup (tests/host_emul/) and
held to the numpy restatement of include/kasf.h's rule (tests/triangulate_ref.py) bit for bit on all five outputs of the triangulation and on the undistortion's
output: at point counts around the triangulation's 128-point tile and the undistortion's 256-point tile, with 2, 3, 7 and 16 views, with 16-byte aligned
pointers and pointers offset by 4 bytes, with static and per-frame cameras, with and without lens distortion, with each optional output null in turn; canaries
around every array, inputs unchanged, no LDS beyond what the launch asked for.  It shows the kernel's logic, its indexing and its fp64 operation order; what only
the device can show stays with tests/test_gpu_triangulate.py."""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build, vp
from tests.triangulate_ref import DEFAULTS, LENS, bundle, holds_every_case, same_bits, triangulate_np, undistort_np

OUTPUTS = ("points", "residual", "used", "state", "view_residual")
BYTES = ("used", "state")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "triangulate_host", "emul_triangulate.cpp")
    lib.emul_triangulate.restype = C.c_int
    lib.emul_undistort.restype = C.c_int
    return lib


class Guarded:
    """An array of `shape` whose first element lies `offset` bytes past a multiple of 16, with 64 canary bytes on either side."""

    def __init__(self, shape, dtype, offset=0, data=None, fill=0):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.buf = np.full(self.nbytes + 160, 0x5A, np.uint8)
        self.start = 64 + (-(self.buf.ctypes.data + 64) % 16) + offset
        self.a = self.buf[self.start:self.start + self.nbytes].view(dtype).reshape(shape)
        self.a[...] = fill if data is None else data
        self.keep = self.buf.copy()

    def unchanged(self):
        return np.array_equal(self.buf, self.keep)

    def intact(self):
        return np.array_equal(self.buf[:self.start], self.keep[:self.start]) and np.array_equal(self.buf[self.start + self.nbytes:], self.keep[self.start + self.nbytes:])


def run(emul, K, cams, ppf, offset=0, null=(), **kw):
    """-> {output: array} of the outputs that were asked for; checks the canaries, the inputs and the LDS."""
    q = {**DEFAULTS, **kw}
    views, M = K.shape[:2]
    kin, cin = Guarded(K.shape, np.float32, offset, K), Guarded(cams.shape, np.float32, 0, cams)
    shapes = {"points": (M, 3), "residual": (M,), "used": (M,), "state": (M,), "view_residual": (views, M)}
    outs = {k: Guarded(shapes[k], np.uint8 if k in BYTES else np.float32, offset if k in ("points", "view_residual") else 0, fill=77 if k in BYTES else 9.0)
            for k in OUTPUTS}
    arg = lambda k: None if k in null else vp(outs[k].a)                 # noqa: E731
    overrun = emul.emul_triangulate(vp(kin.a), views, C.c_int64(M), ppf, vp(cin.a), int(cams.ndim == 3), C.c_float(q["min_score"]), int(q["weighted"]),
                                    q["iterations"], C.c_float(q["delta"]), q["min_views"], q["undistort_iterations"], arg("points"), arg("residual"),
                                    arg("used"), arg("state"), arg("view_residual"))
    assert overrun == 0
    assert kin.unchanged() and cin.unchanged()
    assert all(o.intact() for o in outs.values())
    assert all(outs[k].unchanged() for k in null)
    return {k: outs[k].a for k in OUTPUTS if k not in null}


def check(got, want):
    for k, a in got.items():
        assert same_bits(a, want[k]), (k, np.argwhere(a.view(np.uint8).reshape(-1) != want[k].view(np.uint8).reshape(-1))[:4] // a.dtype.itemsize)


@pytest.mark.parametrize("points", [1, 127, 128, 129, 255, 256, 257, 513])
@pytest.mark.parametrize("offset", [0, 4])
def test_point_counts_around_the_tile(emul, points, offset):
    """J = 1: every point a frame of its own, 3 views (an odd M makes views 1 and 2 start off a 16-byte boundary even from an aligned base)."""
    K, cams, _ = bundle(points, 3, seed=points, per_frame=points % 2 == 1, joints=1)
    want = triangulate_np(K, cams, 1)
    check(run(emul, K, cams, 1, offset), want)
    if points >= 127:
        assert holds_every_case(want, 3)


@pytest.mark.parametrize("frames", [1, 15, 16, 31])
@pytest.mark.parametrize("views", [2, 3, 7, 16])
@pytest.mark.parametrize("per_frame", [False, True])
def test_frames_of_seventeen_joints(emul, frames, views, per_frame):
    K, cams, _ = bundle(frames, views, seed=frames + views, per_frame=per_frame)
    assert cams.ndim == 2 + per_frame
    want = triangulate_np(K, cams, 17)
    check(run(emul, K, cams, 17, offset=4 * (frames % 2)), want)
    if frames >= 15 and views >= 3:
        assert holds_every_case(want, views)
    if per_frame and frames > 1:                                         # the rows really differ: frame 0's rows for all give other bits
        assert not same_bits(triangulate_np(K, cams[:, 0], 17)["points"], want["points"])


@pytest.mark.parametrize("rounds", [0, 5, 20])
@pytest.mark.parametrize("lens", [False, True])
def test_lens_distortion_and_rounds(emul, rounds, lens):
    K, cams, _ = bundle(16, 7, seed=40, distortion=LENS if lens else None)
    want = triangulate_np(K, cams, 17, undistort_iterations=rounds)
    check(run(emul, K, cams, 17, undistort_iterations=rounds), want)
    assert 2 * int((want["state"] == 0).sum()) >= len(want["state"])
    if lens and rounds:                                                  # the lens matters: a pinhole reading of the same keypoints gives other bits
        assert not same_bits(triangulate_np(K, cams, 17, undistort_iterations=0)["points"], want["points"])


@pytest.mark.parametrize("iterations", [0, 1, 8])
@pytest.mark.parametrize("weighted", [False, True])
def test_iterations_and_weights(emul, iterations, weighted):
    K, cams, _ = bundle(16, 7, seed=41, distortion=LENS)
    q = dict(iterations=iterations, weighted=weighted, delta=2.5, min_score=0.25)
    want = triangulate_np(K, cams, 17, **q)
    check(run(emul, K, cams, 17, **q), want)
    assert holds_every_case(want, 7)


@pytest.mark.parametrize("null", ["residual", "used", "state", "view_residual"])
def test_each_optional_output_null_in_turn(emul, null):
    K, cams, _ = bundle(16, 3, seed=42)
    got = run(emul, K, cams, 17, null=(null,))
    assert null not in got and len(got) == 4
    check(got, triangulate_np(K, cams, 17))


def test_a_frame_alone_equals_the_frame_in_the_batch(emul):
    K, cams, _ = bundle(31, 7, seed=43, per_frame=True)
    full = run(emul, K, cams, 17)
    for f in (0, 7, 8, 30):                                              # frames 7 and 8 straddle the first tile's end at point 128
        one = run(emul, K[:, 17 * f:17 * f + 17], cams[:, f:f + 1], 17)
        for k in OUTPUTS:
            part = full[k][:, 17 * f:17 * f + 17] if k == "view_residual" else full[k][17 * f:17 * f + 17]
            assert same_bits(one[k], part), (f, k)


@pytest.mark.parametrize("points", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("rounds", [0, 5, 20])
def test_undistort_follows_the_rule(emul, points, offset, rounds):
    per_frame = points % 2 == 1
    K, cams, _ = bundle(points, 3, seed=points + 1, per_frame=per_frame, distortion=LENS, joints=1)
    kp, cam = K[1].copy(), np.ascontiguousarray(cams[1, ..., :9])
    kp[::50, 1] = np.inf                                                 # not usable: copied as it came
    kin, cin = Guarded(kp.shape, np.float32, offset, kp), Guarded(cam.shape, np.float32, 0, cam)
    out = Guarded(kp.shape, np.float32, offset, fill=9.0)
    assert emul.emul_undistort(vp(kin.a), C.c_int64(points), 1, vp(cin.a), int(per_frame), rounds, vp(out.a)) == 0
    assert kin.unchanged() and cin.unchanged() and out.intact()
    want = undistort_np(kp, cam, 1, rounds)
    assert same_bits(out.a, want)
    assert same_bits(want[::50], kp[::50]) and same_bits(want[:, 2], kp[:, 2])
    if rounds and points > 1:
        assert not same_bits(want, kp)
    if per_frame and points > 100:                                       # view 1's camera has a NaN in R now and then, which the lens part does not read
        assert np.isnan(cams[1]).any() and not np.isnan(cam).any()


def test_undistort_with_frames_of_seventeen_joints(emul):
    K, cams, _ = bundle(31, 3, seed=44, per_frame=True, distortion=LENS)
    kp, cam = K[0], np.ascontiguousarray(cams[0, :, :9])
    cam[3, 4] = np.nan                                                   # a camera value that is not finite: its frame's points are copied
    out = Guarded(kp.shape, np.float32, 0, fill=9.0)
    assert emul.emul_undistort(vp(kp), C.c_int64(len(kp)), 17, vp(cam), 1, 5, vp(out.a)) == 0
    want = undistort_np(kp, cam, 17, 5)
    assert out.intact() and same_bits(out.a, want) and same_bits(want[51:68], kp[51:68])
