"""The decoder-surface conversion on the device (kasf_yuv420_to_bgr, K.yuv_to_bgr / nv12_to_bgr / i420_to_bgr) against the numpy restatement of
tests/test_yuv_cpu.py, which that file ties to the exact fp64 conversion over all 2^24 samples.  Device and restatement perform the same integer operations,
so every comparison is exact.  Nothing here provokes a fault: refusals are tested through the error code; no test looks at the kernel's assembly.

The kernel's two forms (csrc/k_yuv.hip), which the placements are chosen by: planes and output on torch's allocation grid behind pitches that are multiples
of 8 take the vector form (2 x 8 blocks, whole-dword loads and stores) with quads for the right / bottom remainders; a slice that starts one byte into its
buffer behind odd pitches takes quads for everything."""
import numpy as np
import pytest
import torch

from tests.gpu_util import ptr, stream
from tests.test_yuv_cpu import ACCEPTED, NULLS, REFUSED, SIZES, TABLES, call_entry, interleave, noise_planes, nv12_to_bgr_np, yuv_to_bgr_np

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 0xEE, 0xC3
COMBOS = [(m, fr, rgb) for (m, fr) in sorted(TABLES) for rgb in (False, True)]


def up(n, a):
    return (n + a - 1) // a * a


def pitched(F, rows, row_bytes, pitch, frame_stride, offset, fill, data=None, pairs=False):
    """A device buffer of `fill` and a strided view into it, `offset` bytes past its start: [F,rows,row_bytes] (or [F,rows,row_bytes / 2,2] with pairs)."""
    buf = torch.full((offset + (F - 1) * frame_stride + rows * pitch + 64,), fill, dtype=torch.uint8, device="cuda")
    view = buf[offset:].as_strided((F, rows, row_bytes), (frame_stride, pitch, 1))
    if data is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(F, rows, row_bytes)))
    if pairs:
        view = buf[offset:].as_strided((F, rows, row_bytes // 2, 2), (frame_stride, pitch, 2, 1))
    return buf, view


def place(y, u, v, layout, where):
    """The planes as strided device views (F = y.shape[0]) and a pitched output full of SENTINEL -> (input views, input buffers, out view, out buffer)."""
    F, Hf, Wf = y.shape
    ch, cw = u.shape[1:]
    nv12 = layout == "nv12"
    crow = 2 * cw if nv12 else cw
    if where == "odd":
        off, yp, cp, op = 1, Wf + 3, crow + 3, 3 * Wf + 5
        yf, cf, of = Hf * yp + 7, ch * cp + 5, Hf * op + 3
    else:
        off, yp, cp, op = 0, up(Wf, 8) + 8, up(crow, 8) + 8, up(3 * Wf, 4) + 4
        yf, cf, of = Hf * yp + 16, ch * cp + 8, Hf * op + 12
    bufs, views = [], []
    for data, rows, rb, p, fs, pairs in ([(y, Hf, Wf, yp, yf, False)] + ([(interleave(u, v), ch, crow, cp, cf, True)] if nv12 else
                                                                       [(u, ch, crow, cp, cf, False), (v, ch, crow, cp, cf, False)])):
        b, w = pitched(F, rows, rb, p, fs, off, PAD, data, pairs)
        bufs.append(b)
        views.append(w)
    obuf, oview = pitched(F, Hf, 3 * Wf, op, of, off, SENTINEL)
    return views, bufs, obuf[off:].as_strided((F, Hf, Wf, 3), (of, op, 3, 1)), obuf


def only_payload_changed(obuf, oview, before):
    now, keep = obuf.clone(), before.clone()
    for b in (now, keep):
        b[oview.storage_offset():].as_strided(oview.shape, oview.stride()).zero_()
    return torch.equal(now, keep)


def want(y, u, v, layout, **kw):
    return yuv_to_bgr_np(y, interleave(u, v), **kw) if layout == "nv12" else yuv_to_bgr_np(y, u, v, layout="i420", **kw)


@pytest.mark.parametrize("where", ["grid", "odd"])
def test_strided_views_are_read_in_place_and_a_pitched_out_is_written_in_place(where, monkeypatch):
    """Every size x layout x F = 1, 3 with the tables and rgb rotating; the entry point is handed the views' own addresses (no copy was made), the output's
    padding and the input buffers survive.  `odd`: a slice one byte into its buffer behind odd pitches (the element form)."""
    import kasportsformer_amd as K
    from kasportsformer_amd import _lib
    lib = _lib.load()
    real, seen = lib.kasf_yuv420_to_bgr, []

    def spy(*a):
        seen.append(a)
        return real(*a)

    monkeypatch.setattr(lib, "kasf_yuv420_to_bgr", spy)
    n = 0
    for Hf, Wf in SIZES:
        for F in (1, 3):
            y, u, v = noise_planes(Hf, Wf, seed=1000 * Hf + Wf, frames=F)
            for layout in ("nv12", "i420"):
                matrix, full_range, rgb = COMBOS[n % len(COMBOS)]
                n += 1
                views, bufs, oview, obuf = place(y, u, v, layout, where)
                keep, before = [b.clone() for b in bufs], obuf.clone()
                args = views if F > 1 else [w[0] for w in views]
                o = oview if F > 1 else oview[0]
                got = K.yuv_to_bgr(*args, layout=layout, matrix=matrix, full_range=full_range, rgb=rgb, out=o)
                assert got is o
                call = seen[-1]
                assert [call[0], call[1]] == [views[0].data_ptr(), views[1].data_ptr()] and call[11] == oview.data_ptr(), "read and written in place"
                assert call[2] == (None if layout == "nv12" else views[2].data_ptr())
                assert (views[0].data_ptr() - bufs[0].data_ptr()) == (1 if where == "odd" else 0)
                case = (Hf, Wf, F, layout, matrix, full_range, rgb)
                assert np.array_equal(oview.cpu().numpy(), want(y, u, v, layout, matrix=matrix, full_range=full_range, rgb=rgb)), case
                assert only_payload_changed(obuf, oview, before), case
                assert all(torch.equal(b, k) for b, k in zip(bufs, keep)), "the planes are only read"
    assert len(seen) == n == 28


def test_packed_host_and_odd_views_give_the_same_frame():
    """Without out= a new packed frame comes back; numpy input is uploaded; a view whose samples are not contiguous is packed first."""
    import kasportsformer_amd as K
    y, u, v = noise_planes(37, 23, seed=5)
    ref = want(y[None], u[None], v[None], "nv12")[0]
    got = K.yuv_to_bgr(y, interleave(u, v))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (37, 23, 3) and got.is_contiguous() and np.array_equal(got.cpu().numpy(), ref)
    dy, du, dv = (torch.from_numpy(a).cuda() for a in (y, u, v))
    assert torch.equal(K.yuv_to_bgr(dy, du, dv, layout="i420"), got)
    assert torch.equal(K.yuv_to_bgr(dy.t().contiguous().t(), torch.stack((du, dv), dim=0).permute(1, 2, 0)), got), "column-major luma, planar pairs: packed first"
    wide = torch.stack((du, dv), dim=-1).repeat_interleave(2, dim=1)[:, ::2]                       # chroma samples four bytes apart
    assert wide.stride(-2) == 4 and torch.equal(K.yuv_to_bgr(dy, wide), got)
    assert torch.equal(K.yuv_to_bgr(dy, du, dv.t().contiguous().t(), layout="i420"), got), "U and V with different strides: packed first"
    assert torch.equal(K.yuv_to_bgr(dy, du, dv, layout="i420", rgb=True), got.flip(-1))
    with pytest.raises(ValueError):
        K.yuv_to_bgr(dy, du, dv, layout="i420", out=torch.empty((37, 23, 3), dtype=torch.uint8, device="cuda").permute(1, 0, 2).contiguous().permute(1, 0, 2))


def surface_1080p():
    g = np.random.default_rng(1080)
    return g.integers(0, 256, size=(1088 + 540, 2048), dtype=np.uint8)


def test_a_full_hd_surface_with_an_aligned_chroma_row():
    """1080 x 1920 NV12 at pitch 2048 with the UV plane at row 1088, as a hardware decoder aligns it; read in place."""
    import kasportsformer_amd as K
    host = surface_1080p()
    dev = torch.from_numpy(host).cuda()
    keep = dev.clone()
    got = K.nv12_to_bgr(dev, 1080, 1920, chroma_row=1088)
    assert tuple(got.shape) == (1080, 1920, 3) and np.array_equal(got.cpu().numpy(), nv12_to_bgr_np(host, 1080, 1920, chroma_row=1088))
    assert torch.equal(dev, keep)
    full = K.nv12_to_bgr(dev, 1080, 1920, chroma_row=1088, matrix="bt709", full_range=True, rgb=True)
    assert np.array_equal(full.cpu().numpy(), nv12_to_bgr_np(host, 1080, 1920, chroma_row=1088, matrix="bt709", full_range=True, rgb=True))


def test_a_frame_does_not_depend_on_the_batch_and_runs_repeat():
    import kasportsformer_amd as K
    y, u, v = noise_planes(37, 23, seed=3, frames=3)
    for layout in ("nv12", "i420"):
        planes = [torch.from_numpy(a).cuda() for a in ((y, interleave(u, v)) if layout == "nv12" else (y, u, v))]
        all_ = K.yuv_to_bgr(*planes, layout=layout)
        again = K.yuv_to_bgr(*planes, layout=layout)
        assert tuple(all_.shape) == (3, 37, 23, 3) and torch.equal(all_, again), "two runs, the same bits"
        assert np.array_equal(all_.cpu().numpy(), want(y, u, v, layout))
        for f in range(3):
            assert torch.equal(K.yuv_to_bgr(*(p[f] for p in planes), layout=layout), all_[f]), (layout, f)
        assert torch.equal(K.yuv_to_bgr(*(p[::2] for p in planes), layout=layout), all_[::2]), "a frame stride of two frames is read in place"


def test_surfaces_of_both_layouts():
    import kasportsformer_amd as K
    y, u, v = noise_planes(36, 40, seed=8)
    ref = yuv_to_bgr_np(y, u, v, layout="i420")
    packed = np.concatenate((y.reshape(-1), u.reshape(-1), v.reshape(-1))).reshape(54, 40)                 # yuv420p in one buffer
    assert np.array_equal(K.i420_to_bgr(torch.from_numpy(packed).cuda()).cpu().numpy(), ref)
    assert np.array_equal(K.i420_to_bgr(packed).cpu().numpy(), ref), "host input is uploaded"
    semi = np.concatenate((y, interleave(u, v).reshape(18, 40)))                                           # PyAV's to_ndarray(format="nv12")
    assert np.array_equal(K.nv12_to_bgr(torch.from_numpy(semi).cuda()).cpu().numpy(), ref)
    both = torch.from_numpy(np.stack((semi, semi[::-1].copy()))).cuda()
    assert torch.equal(K.nv12_to_bgr(both)[0], K.nv12_to_bgr(both[0]))


def test_the_frame_is_what_the_letterbox_and_the_crop_take():
    """The converted frame is used in place by the two kernels behind it, and gives what the restatement's frame gives, bit for bit."""
    import kasportsformer_amd as K
    g = np.random.default_rng(17)
    s = g.integers(0, 256, size=(135, 120), dtype=np.uint8)                                                # 90 x 120 NV12
    frame = K.nv12_to_bgr(torch.from_numpy(s).cuda())
    host = nv12_to_bgr_np(s)
    assert tuple(frame.shape) == (90, 120, 3) and np.array_equal(frame.cpu().numpy(), host)
    assert torch.equal(K.letterbox_frames(frame, 64).inputs, K.letterbox_frames(host, 64).inputs)
    boxes = torch.tensor([[10.0, 5.0, 60.0, 85.0], [70.5, 20.25, 118.0, 88.0]])
    a, b = K.crop_persons(frame, boxes, size=(48, 64)), K.crop_persons(host, boxes, size=(48, 64))
    assert torch.equal(a.inputs, b.inputs) and torch.equal(a.center, b.center) and torch.equal(a.scale, b.scale)
    out = torch.full((90, 512), SENTINEL, dtype=torch.uint8, device="cuda")                                # a pitched frame, written and then read through its pitch
    view = out.as_strided((90, 120, 3), (512, 3, 1))
    K.nv12_to_bgr(torch.from_numpy(s).cuda(), out=view)
    assert bool((out[:, 360:] == SENTINEL).all()) and torch.equal(K.letterbox_frames(view, 64).inputs, K.letterbox_frames(host, 64).inputs)


def test_no_host_synchronisation():
    import kasportsformer_amd as K
    y, u, v = noise_planes(37, 23, seed=6)
    dy, duv = torch.from_numpy(y).cuda(), torch.from_numpy(interleave(u, v)).cuda()
    K.yuv_to_bgr(dy, duv)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    raised, got = False, None
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:                                                                    # the control: a device-to-host copy
            dy.cpu()
        except RuntimeError:
            raised = True
        if raised:
            got = K.yuv_to_bgr(dy, duv)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not raised:
        pytest.skip("this torch build does not raise on a device-to-host copy under set_sync_debug_mode('error'): the check would pass vacuously")
    assert np.array_equal(got.cpu().numpy(), yuv_to_bgr_np(y, interleave(u, v)))


def test_no_frames_is_no_work_and_refusals_launch_nothing():
    """n_frames = 0 leaves a pre-filled output alone; every error-2 refusal of tests/test_yuv_cpu.REFUSED with NULL device pointers (a refusal that looked at one
    would fault; the message names the argument, so the null check did not answer in its place), then with device buffers that must not change."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    planes = torch.full((256,), 3, dtype=torch.uint8, device="cuda")
    out = torch.full((256,), 7, dtype=torch.uint8, device="cuda")
    p, o = ptr(planes), ptr(out)
    assert call_entry(lib, p, p, p, o, stream(), n_frames=0) == 0
    for kw, word in REFUSED:
        assert call_entry(lib, None, None, p, None, stream(), **kw) == 2 and word in lib.kasf_last_error().decode(), (kw, lib.kasf_last_error())
        assert call_entry(lib, p, p, p, o, stream(), **kw) == 2 and word in lib.kasf_last_error().decode(), (kw, lib.kasf_last_error())
    for i, name in enumerate(NULLS):
        ptrs = [p, p, o]
        ptrs[i] = None
        assert call_entry(lib, ptrs[0], ptrs[1], p, ptrs[2], stream()) == 2 and "null pointer" in lib.kasf_last_error().decode(), name
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((planes == 3).all())
    assert call_entry(lib, p, p, p, o, stream()) == 0                             # the accepted call itself: two frames of 5 x 7 behind their pitches
    torch.cuda.synchronize()
    flat = np.full((2, 5, 7), 3, np.uint8)
    ref = yuv_to_bgr_np(flat, np.full((2, 3, 4, 2), 3, np.uint8))
    got = out.cpu().numpy()
    a = ACCEPTED
    for f in range(2):
        rows = np.lib.stride_tricks.as_strided(got[f * a["out_frame_stride"]:], shape=(5, 21), strides=(a["out_row_stride"], 1))
        assert np.array_equal(rows.reshape(5, 7, 3), ref[f])
    assert (got[2 * a["out_frame_stride"]:] == 7).all() and bool((planes == 3).all())
