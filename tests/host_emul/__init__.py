"""What the host-compiled kernel tests (tests/test_*_host_cpu.py, tests/test_host_emul_cpu.py) share, not a test: ``build`` compiles one entry file of this
directory with g++ -- hip/hip_runtime.h here stands in for HIP's, csrc/kernels.h and the kernel's source are the real ones -- and the byte planes with canaries
that the frame kernels' tests lay their buffers out in."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(os.path.dirname(HERE)), "kasportsformer_amd", "csrc")
CANARY, PAD, SENTINEL = 0x5A, 0xEE, 0xC3


def build(tmp_path_factory, name, entry, copy=(), generate={}):
    """tests/host_emul/<entry> as a shared library in a fresh directory `name` -> ctypes.CDLL.  Includes resolve in the build directory, then here, then in csrc;
    `copy` names csrc files to put into the build directory first (a copy's quoted includes then find the stand-ins here before their real neighbours) and
    `generate` maps file names to text to write there.  Skips without g++ or without its C++20 <barrier>."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp(name)
    for f in copy:
        shutil.copy(os.path.join(CSRC, f), d)
    for f, text in generate.items():
        (d / f).write_text(text)
    r = subprocess.run([gxx, "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++", "-I.", "-I" + HERE, "-I" + CSRC, os.path.join(HERE, entry),
                        "-o", "libemul.so", "-lpthread"], cwd=d, capture_output=True, text=True)
    if r.returncode != 0 and "barrier" in r.stderr and "No such file" in r.stderr:
        pytest.skip("this g++ has no C++20 <barrier>")
    assert r.returncode == 0, r.stderr
    return C.CDLL(str(d / "libemul.so"))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def up(n, a):
    return (n + a - 1) // a * a


class Plane:
    """F x rows x row_bytes behind a pitch and a frame stride, `offset` bytes past a multiple of 16, `fill` in the padding, 64 canary bytes on either side."""

    def __init__(self, F, rows, row_bytes, pitch, frame_stride, offset, fill, data=None):
        self.n = (F - 1) * frame_stride + (rows - 1) * pitch + row_bytes
        self.buf = np.full(self.n + 160, CANARY, np.uint8)
        self.start = 64 + (-(self.buf.ctypes.data + 64) % 16) + offset
        self.buf[self.start:self.start + self.n] = fill
        self.view = np.lib.stride_tricks.as_strided(self.buf[self.start:], shape=(F, rows, row_bytes), strides=(frame_stride, pitch, 1))
        if data is not None:
            self.view[:] = data.reshape(F, rows, row_bytes)
        self.keep = self.buf.copy()
        self.ptr, self.pitch, self.frame_stride = self.buf.ctypes.data + self.start, pitch, frame_stride

    def unchanged(self):
        return np.array_equal(self.buf, self.keep)

    def only_payload_changed(self):
        """Everything but the rows' payload -- canaries, row padding, the gaps between frames -- is as it was."""
        now = self.buf.copy()
        for b in (now, self.keep):
            np.lib.stride_tricks.as_strided(b[self.start:], shape=self.view.shape, strides=self.view.strides)[:] = 0
        return np.array_equal(now, self.keep)
