"""csrc/k_letterbox.hip without a GPU: the kernel's own source compiled for the host with g++ behind a lockstep emulation of a workgroup
(tests/host_emul/: one host thread per GPU thread, a barrier at every __syncthreads, the dynamic LDS a buffer of exactly the bytes the launch asks for)
and held to the numpy restatement of include/kasf.h's rules (tests/test_letterbox_cpu.py, letterbox_np), exactly.  It shows the kernel's logic, its indexing
(canaries around the output, the frame and the LDS) and its integer / fp32 / fp64 operation order; what only the device can show stays with
tests/test_gpu_letterbox.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.host_emul import build
from tests.test_letterbox_cpu import ODD_SIZES, fixture, fixture_frame, letterbox_np, noise_frame, plan_np

CANARY = 0x5A
DTYPES = {"fp32": (0, 4, torch.float32), "bf16": (1, 2, torch.bfloat16), "fp16": (2, 2, torch.float16)}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "letterbox_host", "emul_letterbox.cpp")
    lib.emul_letterbox.restype = C.c_int
    lib.emul_letterbox.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p] + [C.c_int] * 9
    return lib


def aligned(nbytes, offset):
    """A uint8 buffer of CANARY with 64 bytes in front of and behind a payload of nbytes whose address is `offset` past a multiple of 16 -> (buffer, start)."""
    buf = np.full(nbytes + 160, CANARY, np.uint8)
    start = 64 + (-(buf.ctypes.data + 64) % 16) + offset
    return buf, start


def run(emul, frames, inp_dim, dtype="fp32", pad=128, swap_rb=True, pitch=None, offset=0):
    """The emulated launch on frames [F,Hf,Wf,3] uint8 (copied behind `pitch` bytes per row, padding 255, canaries around) -> the output as a torch tensor
    [F,3,out_h,out_w]; asserts that nothing outside the output changed and the frame buffer did not change at all."""
    frames = np.asarray(frames)
    frames = frames if frames.ndim == 4 else frames[None]
    F, Hf, Wf = frames.shape[:3]
    out_w, out_h = (inp_dim, inp_dim) if isinstance(inp_dim, int) else inp_dim
    new_w, new_h, pad_x, pad_y = plan_np(Wf, Hf, out_w, out_h)
    pitch = 3 * Wf if pitch is None else pitch
    fbuf, fs = aligned(F * Hf * pitch, 1)                                          # frames at an odd address: bytes have no alignment to rely on
    fbuf[fs:fs + F * Hf * pitch] = 255
    view = np.lib.stride_tricks.as_strided(fbuf[fs:], shape=(F, Hf, Wf, 3), strides=(Hf * pitch, pitch, 3, 1))
    view[:] = frames
    keep = fbuf.copy()
    code, esize, tdt = DTYPES[dtype]
    n = F * 3 * out_h * out_w * esize
    obuf, os_ = aligned(n, offset)
    over = emul.emul_letterbox(fbuf.ctypes.data + fs, F, Hf, Wf, pitch, Hf * pitch if F > 1 else 0, obuf.ctypes.data + os_, code, out_w, out_h, new_w, new_h,
                               pad_x, pad_y, pad, int(swap_rb))
    assert over == 0, "a workgroup wrote past its dynamic LDS"
    assert np.array_equal(fbuf, keep), "the frame is only read"
    assert (obuf[:os_] == CANARY).all() and (obuf[os_ + n:] == CANARY).all(), "nothing outside the output is written"
    return torch.frombuffer(bytearray(obuf[os_:os_ + n].tobytes()), dtype=tdt).reshape(F, 3, out_h, out_w)


def same(got, want_np):
    return torch.equal(got, torch.from_numpy(want_np).to(got.dtype))


@pytest.mark.parametrize("name,pitch", [("land", 400), ("port", 304)])
def test_kernel_source_on_the_fixture_frames_through_their_pitch(emul, name, pitch):
    fx = fixture()
    frame = fixture_frame(fx, name)
    for dim in (64, 32):
        got = run(emul, frame, dim, pitch=pitch)
        assert np.array_equal(got.numpy().view(np.uint32), fx[f"{name}_prep_{dim}"].view(np.uint32)), "the reference's bookkeeping, bit for bit"
    for size in ODD_SIZES:
        assert same(run(emul, frame, size, pitch=pitch), letterbox_np(frame, size)), size
    assert same(run(emul, frame, 64, pitch=pitch, offset=4), letterbox_np(frame, 64)), "an output off the 16-byte grid takes element stores"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_sixteen_bit_outputs_round_the_fp32_result(emul, dtype):
    frame = fixture_frame(fixture(), "port")
    for size, offset in ((64, 0), ((48, 32), 0), ((12, 8), 0), ((33, 31), 0), (64, 2)):         # (33, 31) and an output 2 bytes off the grid: element stores
        assert same(run(emul, frame, size, dtype=dtype, pitch=304, offset=offset), letterbox_np(frame, size)), (size, offset)


def test_upscale_identity_and_tiny_frames(emul):
    up = noise_frame(30, 40, seed=5)
    assert same(run(emul, up, 96), letterbox_np(up, 96))
    ident = noise_frame(64, 64, seed=3)
    got = run(emul, ident, 64)
    assert same(got, letterbox_np(ident, 64)) and torch.equal(got[0], torch.from_numpy(ident[:, :, ::-1].transpose(2, 0, 1).copy()).float() / 255)
    for Hf, Wf in ((1, 1), (3, 2), (5, 7)):
        tiny = noise_frame(Hf, Wf, seed=Hf + 10)
        for size in (8, (12, 8), (5, 3)):
            assert same(run(emul, tiny, size), letterbox_np(tiny, size)), (Hf, Wf, size)


def test_batch_parameters_and_padding(emul):
    frames = np.stack([noise_frame(21, 34, seed=s) for s in range(3)])
    all_ = run(emul, frames, (40, 24), pitch=108)
    assert same(all_, letterbox_np(frames, (40, 24)))
    for f in range(3):
        assert torch.equal(run(emul, frames[f], (40, 24))[0], all_[f]), "a frame's planes are a function of that frame alone"
    plain = run(emul, frames[0], (40, 24), swap_rb=False)
    assert torch.equal(plain.flip(1)[0], all_[0]) and same(plain, letterbox_np(frames[0], (40, 24), swap_rb=False))
    for pad in (0, 255):
        got = run(emul, frames[0], 32, pad=pad)
        assert same(got, letterbox_np(frames[0], 32, pad=pad)) and bool((got[0, :, 0] == pad / 255).all())
