"""csrc/k_place.hip without a GPU: the kernel's own source compiled for the host with g++ behind a lockstep emulation of a workgroup (tests/host_emul/) and held
to the numpy restatement of include/kasf.h's rule (tests/place_ref.py) bit for bit on all five outputs: at sizes around the 64-frame tile, with 16-byte aligned
pointers and with pointers offset by 4 bytes, with the camera and the table as one row and per frame, with each optional output null in turn; canaries around
every array, inputs unchanged, no LDS beyond the kernel's own.  It shows the kernel's logic, its indexing and its fp64 operation order; what only the device can
show stays with tests/test_gpu_place.py."""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build, vp
from tests.place_ref import bundle, place_np, same_bits

OUTPUTS = ("poses", "root", "residual", "scale", "state")
FILL = {"poses": 9.0, "root": 9.0, "residual": 9.0, "scale": 9.0, "state": 77}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "place_host", "emul_place.cpp")
    lib.emul_place.restype = C.c_int
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


def run(emul, P, K, camera, lengths, offset=0, null=(), **kw):
    """-> {output: array} of the outputs that were asked for; checks the canaries, the inputs and the LDS."""
    q = {**dict(min_score=0.3, weighted=True, iterations=4, delta=3.0, min_joints=4), **kw}
    N = len(P)
    pin, kin = Guarded(P.shape, np.float32, offset, P), Guarded(K.shape, np.float32, offset, K)
    cin = Guarded(camera.shape, np.float32, 0, camera)
    lin = Guarded(lengths.shape, np.float32, 0, lengths) if lengths is not None else None
    shapes = {"poses": (N, 17, 3), "root": (N, 3), "residual": (N,), "scale": (N,), "state": (N,)}
    outs = {k: Guarded(shapes[k], np.uint8 if k == "state" else np.float32, offset if k == "poses" else 0, fill=FILL[k]) for k in OUTPUTS}
    arg = lambda k: None if k in null else vp(outs[k].a)                 # noqa: E731
    overrun = emul.emul_place(vp(pin.a), vp(kin.a), C.c_int64(N), vp(cin.a), int(camera.ndim == 2), vp(lin.a) if lin is not None else None,
                              int(lengths is not None and lengths.ndim == 2), C.c_float(q["min_score"]), int(q["weighted"]), q["iterations"], C.c_float(q["delta"]),
                              q["min_joints"], arg("poses"), arg("root"), arg("residual"), arg("scale"), arg("state"))
    assert overrun == 0
    assert pin.unchanged() and kin.unchanged() and cin.unchanged() and (lin is None or lin.unchanged())
    assert all(o.intact() for o in outs.values())
    assert all(outs[k].unchanged() for k in null)
    return {k: outs[k].a for k in OUTPUTS if k not in null}


def check(got, want):
    for k, a in got.items():
        assert same_bits(a, want[k]), (k, np.argwhere(a.view(np.uint8).reshape(len(a), -1) != want[k].view(np.uint8).reshape(len(a), -1))[:4])


@pytest.mark.parametrize("frames", [1, 63, 64, 65, 127, 128, 129, 300])
@pytest.mark.parametrize("offset", [0, 4])
def test_kernel_source_follows_the_rule(emul, frames, offset):
    P, K, camera, lengths = bundle(frames, seed=frames)
    want = place_np(P, K, camera, lengths)
    check(run(emul, P, K, camera, lengths, offset), want)
    if frames >= 127:
        assert set(np.unique(want["state"]).tolist()) == {0, 1, 2, 3}
    assert np.isnan(want["poses"][want["state"] != 0]).all() and np.isfinite(want["root"][want["state"] == 0]).all()


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("per_frame", [False, True])
def test_camera_and_table_as_one_row_and_per_frame(emul, table, per_frame):
    P, K, camera, lengths = bundle(129, seed=5, table=table, per_frame=per_frame)
    assert camera.ndim == 1 + per_frame and (lengths is None) == (not table)
    want = place_np(P, K, camera, lengths)
    check(run(emul, P, K, camera, lengths), want)
    if per_frame:                                                        # the rows really differ: one row for all gives other bits
        assert not same_bits(place_np(P, K, camera[0], lengths)["root"], want["root"])


@pytest.mark.parametrize("iterations", [0, 1, 8])
@pytest.mark.parametrize("weighted", [False, True])
def test_iterations_and_weights(emul, iterations, weighted):
    P, K, camera, lengths = bundle(129, seed=8)
    q = dict(iterations=iterations, weighted=weighted, delta=2.5, min_joints=6, min_score=0.25)
    check(run(emul, P, K, camera, lengths, **q), place_np(P, K, camera, lengths, **q))


@pytest.mark.parametrize("null", ["root", "residual", "scale", "state"])
def test_each_optional_output_null_in_turn(emul, null):
    P, K, camera, lengths = bundle(70, seed=9)
    got = run(emul, P, K, camera, lengths, null=(null,))
    assert null not in got and len(got) == 4
    check(got, place_np(P, K, camera, lengths))


def test_a_frame_alone_equals_the_frame_in_the_batch(emul):
    P, K, camera, lengths = bundle(129, seed=10, per_frame=True)
    full = run(emul, P, K, camera, lengths)
    for f in (0, 64, 128):
        one = run(emul, P[f:f + 1], K[f:f + 1], camera[f:f + 1], lengths[f:f + 1])
        for k in OUTPUTS:
            assert same_bits(one[k], full[k][f:f + 1]), (f, k)
