"""The detector's letterbox on the device (kasf_letterbox_frames, K.letterbox_frames) against the numpy restatement of tests/test_letterbox_cpu.py, which that
file ties to the reference's own letterbox_image / prep_image bookkeeping and to exact cubic convolution.  Device and restatement perform the same integer
and IEEE operations, so every comparison is exact (torch.equal).  Nothing here provokes a fault: refusals are tested through the error code; no test looks
at the kernel's assembly.

The kernel's paths (csrc/k_letterbox.hip), which the sizes are chosen by: a thread stores four pixels per plane at once (16 bytes of fp32, 8 of fp16 / bf16)
when the input's width is a multiple of four and the output is aligned to that store -- 64 and 416 in all three types, (12, 8), (48, 32), (40, 24) --, one
element otherwise ((33, 31), (5, 3)); the four taps of a row are read as one 12-byte window, whose weights carry the clamp at the frame's edges, and byte by
byte in frames of fewer than four columns (1 x 1, 2 x 3); one workgroup walks one chunk of 256 such groups per frame, four once frames x chunks exceeds
2,048 (never at these sizes: the grid-stride loop is the same code)."""
import numpy as np
import pytest
import torch

from tests.gpu_util import ptr, stream
from tests.test_letterbox_cpu import F32, REFUSED, fixture, fixture_frame, letterbox_np, noise_frame, plan_np

pytestmark = pytest.mark.gpu

_SHARED = {}


def golden():
    """The fixture, its two frames on the device through their padded pitch -- once."""
    if not _SHARED:
        fx = fixture()
        g = {}
        for name in ("land", "port"):
            host = fixture_frame(fx, name)
            buf = torch.from_numpy(fx[name + "_buf"].copy()).cuda()                            # [Hf, pitch]
            Hf, Wf = host.shape[:2]
            g[name] = (host, buf.as_strided((Hf, Wf, 3), (buf.stride(0), 3, 1)), buf)
            for dim in (64, 32):
                g[f"{name}_prep_{dim}"] = fx[f"{name}_prep_{dim}"]
        _SHARED.update(g)
    return _SHARED


def equal(got: torch.Tensor, want_np) -> bool:
    want = torch.from_numpy(want_np)
    return got.shape == want.shape and torch.equal(got.cpu(), want.to(got.dtype))


@pytest.mark.parametrize("name", ["land", "port"])
def test_fixture_frames_through_their_pitch(name):
    """Landscape pads top and bottom, portrait left and right; the frame is read through its padded pitch (padding bytes are 255: a read into them would
    show against the restatement, which never sees them) and is unchanged afterwards."""
    import kasportsformer_amd as K
    g = golden()
    host, dev, buf = g[name]
    keep = buf.clone()
    assert not dev.is_contiguous() and bool((buf[:, 3 * host.shape[1]:] == 255).all())
    for dim in (64, 32):
        r = K.letterbox_frames(dev, dim)
        assert isinstance(r, K.LetterboxResult) and r.inputs.is_cuda and r.inputs.dtype == torch.float32 and tuple(r.inputs.shape) == (1, 3, dim, dim)
        assert torch.equal(r.inputs.cpu(), torch.from_numpy(g[f"{name}_prep_{dim}"])), "the reference's prep_image around the restated resize, bit for bit"
        new_w, new_h, pad_x, pad_y = plan_np(host.shape[1], host.shape[0], dim, dim)
        assert (r.width, r.height) == (host.shape[1], host.shape[0]) and r.size == (new_w, new_h) and r.offset == (pad_x, pad_y)
        assert (pad_y > 0 and pad_x == 0) if name == "land" else (pad_x > 0 and pad_y == 0)
        inside = torch.zeros((dim, dim), dtype=torch.bool)
        inside[pad_y:pad_y + new_h, pad_x:pad_x + new_w] = True
        assert bool((r.inputs.cpu()[0][:, ~inside] == np.float32(128) / np.float32(255)).all())
    r = K.letterbox_frames(dev, (48, 32))
    assert tuple(r.inputs.shape) == (1, 3, 32, 48) and equal(r.inputs, letterbox_np(host, (48, 32)))
    assert torch.equal(buf, keep), "the frame is only read"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_store_paths_and_sixteen_bit_outputs(dtype):
    import kasportsformer_amd as K
    g = golden()
    host, dev, _ = g["port"]
    for size in (64, (33, 31), (5, 3), (12, 8)):                               # 64 and (12, 8): four-pixel stores; the others element stores
        want = letterbox_np(host, size)
        full = K.letterbox_frames(dev, size)
        assert equal(full.inputs, want), size
        r = K.letterbox_frames(dev, size, dtype=dtype)
        assert r.inputs.dtype == dtype and torch.equal(r.inputs, full.inputs.to(dtype)), size


def test_upscale_identity_and_tiny_frames():
    import kasportsformer_amd as K
    up = noise_frame(30, 40, seed=5)
    assert equal(K.letterbox_frames(up, 96).inputs, letterbox_np(up, 96))
    ident = noise_frame(64, 64, seed=3)
    r = K.letterbox_frames(ident, 64)
    assert r.size == (64, 64) and r.offset == (0, 0) and equal(r.inputs, letterbox_np(ident, 64))
    assert torch.equal(r.inputs[0].cpu(), torch.from_numpy(ident[:, :, ::-1].transpose(2, 0, 1).copy()).float() / 255), "nothing resized: the frame itself"
    for Hf, Wf in ((1, 1), (3, 2), (5, 7)):                                      # every tap clamps
        tiny = noise_frame(Hf, Wf, seed=Hf + 10)
        for size in (8, (12, 8), (5, 3)):
            assert equal(K.letterbox_frames(tiny, size).inputs, letterbox_np(tiny, size)), (Hf, Wf, size)


def test_full_hd_to_the_network_size():
    """1080 x 1920 -> 416, once: where a position formed in fp32 instead of fp64 first shows."""
    import kasportsformer_amd as K
    frame = noise_frame(1080, 1920, seed=1080)
    r = K.letterbox_frames(torch.from_numpy(frame).cuda(), 416)
    assert r.size == (416, 234) and r.offset == (0, 91) and equal(r.inputs, letterbox_np(frame, 416))
    half = K.letterbox_frames(torch.from_numpy(frame).cuda(), 416, dtype=torch.float16)
    assert torch.equal(half.inputs, r.inputs.half())


def test_a_frame_does_not_depend_on_the_batch_and_runs_repeat():
    import kasportsformer_amd as K
    frames = np.stack([noise_frame(21, 34, seed=s) for s in range(3)])
    dev = torch.from_numpy(frames).cuda()
    all_ = K.letterbox_frames(dev, (40, 24))
    again = K.letterbox_frames(dev, (40, 24))
    assert tuple(all_.inputs.shape) == (3, 3, 24, 40) and torch.equal(all_.inputs, again.inputs), "two runs, the same bits"
    assert equal(all_.inputs, letterbox_np(frames, (40, 24)))
    for f in range(3):
        assert torch.equal(K.letterbox_frames(dev[f], (40, 24)).inputs[0], all_.inputs[f]), f
    pitched = torch.full((3, 21, 120), 255, dtype=torch.uint8, device="cuda")            # frames behind a pitch and a frame stride
    view = pitched.as_strided((3, 21, 34, 3), (21 * 120, 120, 3, 1))
    view.copy_(dev)
    assert torch.equal(K.letterbox_frames(view, (40, 24)).inputs, all_.inputs)
    assert torch.equal(K.letterbox_frames(dev[::2], (40, 24)).inputs, all_.inputs[::2]), "a frame stride of two frames is read in place"


def test_pitched_view_equals_its_packed_copy_and_host_input():
    import kasportsformer_amd as K
    g = golden()
    host, view, _ = g["land"]
    packed = view.contiguous()
    a, b = K.letterbox_frames(view, 64), K.letterbox_frames(packed, 64)
    assert torch.equal(a.inputs, b.inputs)
    from_host = K.letterbox_frames(host, 64)                                                # numpy view on the host: uploaded
    assert from_host.inputs.is_cuda and torch.equal(from_host.inputs, a.inputs)
    assert torch.equal(K.letterbox_frames(torch.from_numpy(np.ascontiguousarray(host)), 64).inputs, a.inputs)
    planar = packed.permute(2, 0, 1).contiguous().permute(1, 2, 0)                          # [Hf,Wf,3] over planar storage: packed first
    assert planar.stride(-1) != 1 and torch.equal(K.letterbox_frames(planar, 64).inputs, a.inputs)


def test_swap_and_pad_parameters():
    import kasportsformer_amd as K
    g = golden()
    host, dev, _ = g["land"]
    swapped = K.letterbox_frames(dev, 64)
    plain = K.letterbox_frames(dev, 64, swap_rb=False)
    assert torch.equal(plain.inputs.flip(1), swapped.inputs) and equal(plain.inputs, letterbox_np(host, 64, swap_rb=False))
    for pad in (0, 255):
        r = K.letterbox_frames(dev, 64, pad=pad)
        assert equal(r.inputs, letterbox_np(host, 64, pad=pad))
        assert bool((r.inputs[0, :, 0] == pad / 255).all()) and bool((r.inputs[0, :, -1] == pad / 255).all()), "the first and last rows are padding"


def test_no_frames_is_no_work_and_refusals_launch_nothing():
    """n_frames = 0 leaves a pre-filled output alone; every error-2 refusal of tests/test_letterbox_cpu.REFUSED with device buffers: the code comes back,
    nothing is launched, no buffer changes."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    frame, out = torch.full((2 * 5 * 7 * 3,), 3, dtype=torch.uint8, device="cuda"), torch.full((2 * 3 * 4 * 6,), 7.0, device="cuda")

    def call(frames=ptr(frame), n_frames=1, Hf=5, Wf=7, row_stride=21, frame_stride=105, out=ptr(out), dtype=0, out_w=6, out_h=4, pad=128, swap=1):
        return lib.kasf_letterbox_frames(frames, n_frames, Hf, Wf, row_stride, frame_stride, out, dtype, out_w, out_h, pad, swap, stream())

    assert call(n_frames=0) == 0
    for kw in REFUSED:
        assert call(**kw) == 2 and lib.kasf_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((frame == 3).all())
    assert call(n_frames=2) == 0                                                 # the same arguments, accepted: every element is written
    torch.cuda.synchronize()
    want = letterbox_np(np.full((2, 5, 7, 3), 3, np.uint8), (6, 4))
    assert torch.equal(out.view(2, 3, 4, 6).cpu(), torch.from_numpy(want)) and bool((frame == 3).all())
    assert F32(3) / F32(255) in want and F32(128) / F32(255) in want
