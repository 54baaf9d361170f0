"""The person crop on the device (kasf_crop_persons, K.crop_persons) against the numpy restatement of tests/test_crop_cpu.py, which that file ties to the
reference's center / scale / forward matrix, to torch's normalisation and to exact bilinear sampling.  Device and restatement perform the same integer and
IEEE operations, so every comparison is exact (torch.equal).  Nothing here provokes a fault: refusals are tested through the error code.

The kernel's paths (csrc/k_crop.hip), which the sizes are chosen by: a thread stores 16 bytes per plane (4 fp32 / 8 fp16 or bf16 pixels) when the crop's
width is a multiple of that and the output is 16-byte aligned -- 24 x 32 and 288 x 384 in all three types --, one element otherwise (33 x 31, 5 x 3; 12 x 8 in
the 16-bit types); one workgroup walks one chunk of 256 such groups per person, four once persons x chunks exceeds 2,048 (the 288 x 384 crop of 20 persons)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import ptr, stream
from tests.test_crop_cpu import F32, MEAN, REFUSED, STD, crop_persons_np, fixture, fixture_frames
from tests.test_heatmap_cpu import heatmap_decode_np

pytestmark = pytest.mark.gpu

_SHARED = {}


def golden():
    """The fixture, its two frames on the device through the padded pitch, and the restatement's result for the fixture's persons on the noisy frame -- computed once."""
    if not _SHARED:
        fx = fixture()
        g = {k: fx[k] for k in fx.files}
        g["host_frames"] = fixture_frames(fx)
        buf = torch.from_numpy(g["frames"].copy()).cuda()                                   # [2, Hf, pitch]
        Hf, Wf = g["host_frames"].shape[1:3]
        g["dev_frames"] = buf.as_strided((2, Hf, Wf, 3), (buf.stride(0), buf.stride(1), 3, 1))
        g["buffer"] = buf
        g["out_size"] = tuple(int(v) for v in g["size"])
        g["want"] = crop_persons_np(g["host_frames"][1], g["boxes"], size=g["out_size"])
        _SHARED.update(g)
    return _SHARED


def random_boxes(n, Hf, Wf, seed):
    g = np.random.default_rng(seed)
    cx, cy = g.uniform(-0.1 * Wf, 1.1 * Wf, n), g.uniform(-0.1 * Hf, 1.1 * Hf, n)
    bw, bh = g.uniform(0.02, 0.6, n) * Wf, g.uniform(0.05, 0.9, n) * Hf
    return np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), axis=-1).astype(F32)


def same(got: torch.Tensor, want) -> bool:
    want = torch.as_tensor(want).to(got.device)
    return got.shape == want.shape and torch.equal(got.isnan(), want.isnan()) and torch.equal(torch.where(got.isnan(), 0.0, got), torch.where(want.isnan(), 0.0, want))


@pytest.mark.parametrize("kind", ["box", "center_scale"])
def test_fixture_crops_to_the_restatement(kind):
    """Inside, over each edge, fully outside, larger than the frame, zero width, zero size, center x == -1, a NaN box, fractional corners, exact half-grid ties;
    the frame is read through its padded pitch (padding bytes are 255: a read into them would show) and is unchanged afterwards."""
    import kasportsformer_amd as K
    g = golden()
    frame, keep = g["dev_frames"][1], g["buffer"].clone()
    want, c, s = g["want"]
    if kind == "box":
        r = K.crop_persons(frame, g["boxes"], size=g["out_size"])
    else:
        r = K.crop_persons(frame, center=torch.from_numpy(g["ref_center"]).cuda(), scale=g["ref_scale"], size=g["out_size"])
    assert isinstance(r, K.CropResult) and r.inputs.is_cuda and r.inputs.dtype == torch.float32 and tuple(r.inputs.shape) == (len(c), 3, 32, 24)
    assert torch.equal(r.inputs.cpu(), torch.from_numpy(want)), [str(n) for n, a, b in zip(g["names"], r.inputs.cpu(), torch.from_numpy(want)) if not torch.equal(a, b)]
    assert same(r.center.cpu(), g["ref_center"]) and same(r.scale.cpu(), g["ref_scale"]), "the reference's box_to_center_scale, bit for bit"
    assert torch.equal(g["buffer"], keep), "the frame is only read"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sixteen_bit_outputs_are_the_rounding_of_the_fp32_result(dtype):
    import kasportsformer_amd as K
    g = golden()
    for size in (g["out_size"], (12, 8), (33, 31)):                              # 16-byte stores; 12 is no multiple of 8 and 33 of nothing: element stores
        full = K.crop_persons(g["dev_frames"][1], g["boxes"], size=size)
        r = K.crop_persons(g["dev_frames"][1], g["boxes"], size=size, dtype=dtype)
        assert r.inputs.dtype == dtype and torch.equal(r.inputs, full.inputs.to(dtype)), size
        assert same(r.center, full.center) and same(r.scale, full.scale)            # the NaN box's center and scale are NaN in both
    assert torch.equal(full.inputs.cpu(), torch.from_numpy(crop_persons_np(g["host_frames"][1], g["boxes"], size=(33, 31))[0]))


def test_center_and_scale_feed_the_heatmap_decode():
    import kasportsformer_amd as K
    g = golden()
    keep = ~np.isnan(g["boxes"]).any(axis=1)
    boxes = g["boxes"][keep]
    r = K.crop_persons(g["dev_frames"][0], boxes, size=g["out_size"])
    hm = torch.from_numpy(np.random.default_rng(3).normal(size=(len(boxes), 17, 8, 6)).astype(F32)).cuda()
    kp = K.heatmaps_to_keypoints(hm, r.center, r.scale)
    assert torch.equal(kp, K.heatmaps_to_keypoints(hm, boxes=boxes, aspect=97 / 131)), "the decode derives the same geometry from the boxes"
    assert torch.equal(kp.cpu(), torch.from_numpy(heatmap_decode_np(hm.cpu().numpy(), r.center.cpu().numpy(), r.scale.cpu().numpy())))


def test_pitched_frame_equals_its_packed_copy_and_host_input():
    import kasportsformer_amd as K
    g = golden()
    view = g["dev_frames"][1]
    assert not view.is_contiguous() and view.stride(0) == 400
    packed = view.contiguous()
    a, b = K.crop_persons(view, g["boxes"], size=g["out_size"]), K.crop_persons(packed, g["boxes"], size=g["out_size"])
    assert torch.equal(a.inputs, b.inputs) and torch.equal(a.inputs.cpu(), torch.from_numpy(g["want"][0]))
    host = K.crop_persons(g["host_frames"][1], torch.from_numpy(g["boxes"]), size=g["out_size"])         # numpy view on the host: uploaded
    assert host.inputs.is_cuda and torch.equal(host.inputs, a.inputs)
    planar = packed.permute(2, 0, 1).contiguous().permute(1, 2, 0)                                       # [Hf,Wf,3] over planar storage: packed first
    assert planar.stride(-1) != 1 and torch.equal(K.crop_persons(planar, g["boxes"], size=g["out_size"]).inputs, a.inputs)


def test_frame_index_picks_each_persons_frame():
    import kasportsformer_amd as K
    g = golden()
    P = len(g["boxes"])
    idx = np.arange(P) % 2
    r = K.crop_persons(g["dev_frames"], g["boxes"], size=g["out_size"], frame_index=idx)
    per_frame = [K.crop_persons(g["dev_frames"][f], g["boxes"], size=g["out_size"]).inputs for f in (0, 1)]
    for p in range(P):
        assert torch.equal(r.inputs[p], per_frame[idx[p]][p]), p
    assert not torch.equal(per_frame[0][0], per_frame[1][0])
    on_device = K.crop_persons(g["dev_frames"], g["boxes"], size=g["out_size"], frame_index=torch.from_numpy(idx).cuda())
    assert torch.equal(on_device.inputs, r.inputs)
    # a frame index out of range cannot be refused without a synchronisation when it lives on the device: that person is an all-border crop
    bad = torch.tensor([0, 2, -1] + [1] * (P - 3), dtype=torch.int32, device="cuda")
    got = K.crop_persons(g["dev_frames"], g["boxes"], size=g["out_size"], frame_index=bad).inputs
    border = K.crop_persons(g["dev_frames"][0], g["boxes"][[6]], size=g["out_size"]).inputs[0]           # "outside"
    assert str(g["names"][6]) == "outside" and torch.equal(got[1], border) and torch.equal(got[2], border) and torch.equal(got[0], per_frame[0][0])
    assert torch.equal(got[3:], per_frame[1][3:])


@pytest.mark.parametrize("size,P", [((288, 384), 1), ((288, 384), 20), ((33, 31), 3), ((5, 3), 3)])
def test_network_size_and_odd_sizes(size, P):
    """One 288 x 384 person (108 workgroups of one chunk), 20 of them (four chunks per workgroup), and widths that are no multiple of a 16-byte store."""
    import kasportsformer_amd as K
    g = golden()
    Hf, Wf = g["host_frames"].shape[1:3]
    boxes = random_boxes(P, Hf, Wf, seed=size[0] + P)
    boxes[0] = (20.5, 10.25, 70.75, 90.5)
    if P == 20:
        frame = g["host_frames"][1][:, :Wf // 2]                                   # another pitch: a view of the left half
        dev = g["dev_frames"][1][:, :Wf // 2]
    else:
        frame, dev = g["host_frames"][1], g["dev_frames"][1]
    r = K.crop_persons(dev, boxes, size=size)
    want, c, s = crop_persons_np(frame, boxes, size=size)
    assert torch.equal(r.inputs.cpu(), torch.from_numpy(want))
    assert torch.equal(r.center.cpu(), torch.from_numpy(c)) and torch.equal(r.scale.cpu(), torch.from_numpy(s))
    if P == 20:
        half = K.crop_persons(dev, boxes, size=size, dtype=torch.float16)
        assert torch.equal(half.inputs, r.inputs.half())


def test_swap_mean_std_and_aspect():
    import kasportsformer_amd as K
    g = golden()
    frame, host = g["dev_frames"][1], g["host_frames"][1]
    size = g["out_size"]
    plain = K.crop_persons(frame, g["boxes"], size=size, swap_rb=False)
    assert torch.equal(plain.inputs.cpu(), torch.from_numpy(crop_persons_np(host, g["boxes"], size=size, swap_rb=False)[0]))
    assert torch.equal(plain.inputs.flip(1).cpu(), torch.from_numpy(g["want"][0])), "swap_rb only reorders the planes: normalisation goes by the frame's channel"
    kw = dict(mean=(0.1, 0.2, 0.3), std=(0.5, 2.0, -1.5), aspect=0.75)
    other = K.crop_persons(frame, g["boxes"], size=size, **kw)
    want, c, s = crop_persons_np(host, g["boxes"], size=size, **kw)
    assert torch.equal(other.inputs.cpu(), torch.from_numpy(want)) and same(other.scale.cpu(), s) and not same(other.scale.cpu(), g["ref_scale"])


def test_extreme_geometry_is_defined():
    """Scales and centers far outside any frame: positions saturate at +-2^61 (rule 2), a non-finite geometry is all border, a negative scale mirrors; every tap
    is bounds-checked, so these are ordinary inputs with a defined result."""
    import kasportsformer_amd as K
    g = golden()
    c = np.array([[60, 50], [60, 50], [1e30, 50], [60, -1e30], [60, 50], [60, 50], [3e38, 3e38], [60, 50], [-1, 50], [65.5, 48.5], [60, 50]], F32)
    s = np.array([[1e30, 1], [3e38, 1], [0.5, 1], [0.5, 1], [-0.5, 1], [1e-40, 1], [1e20, 1], [np.inf, 1], [0.3, 0.4], [1e15, 1], [1e12, 1]], F32)
    for size in (g["out_size"], (5, 3)):
        r = K.crop_persons(g["dev_frames"][1], center=c, scale=s, size=size)
        want, _, _, vs = crop_persons_np(g["host_frames"][1], center=c, scale=s, size=size, parts=True)
        assert torch.equal(r.inputs.cpu(), torch.from_numpy(want)), size
    assert not vs[1].any() and not vs[7].any() and vs[4].any(), "scale_x * 200 = inf: border; a negative scale still samples the frame"


def test_a_person_does_not_depend_on_the_batch_and_runs_repeat():
    import kasportsformer_amd as K
    g = golden()
    frame, size = g["dev_frames"][1], g["out_size"]
    all_ = K.crop_persons(frame, g["boxes"], size=size)
    again = K.crop_persons(frame, g["boxes"], size=size)
    assert torch.equal(all_.inputs, again.inputs) and same(all_.center, again.center) and same(all_.scale, again.scale), "two runs, the same bits"
    for p in range(len(g["boxes"])):
        one = K.crop_persons(frame, g["boxes"][p:p + 1], size=size)
        assert torch.equal(one.inputs[0], all_.inputs[p]) and same(one.center[0], all_.center[p]) and same(one.scale[0], all_.scale[p]), str(g["names"][p])


def test_no_persons_is_no_work():
    import kasportsformer_amd as K
    from kasportsformer_amd import _lib
    g = golden()
    r = K.crop_persons(g["dev_frames"][0], np.zeros((0, 4), F32), size=(5, 3), dtype=torch.bfloat16)
    assert tuple(r.inputs.shape) == (0, 3, 3, 5) and r.inputs.is_cuda and tuple(r.center.shape) == tuple(r.scale.shape) == (0, 2)
    out, cs = torch.full((3 * 4 * 6,), 7.0, device="cuda"), torch.full((4,), 9.0, device="cuda")
    frame, geom = torch.zeros(5 * 7 * 3, dtype=torch.uint8, device="cuda"), torch.ones(4, device="cuda")
    ms = (C.c_float * 6)(*MEAN, *STD)
    assert _lib.load().kasf_crop_persons(ptr(frame), 1, 5, 7, 21, 105, None, ptr(geom), 0, 1.0, 0, ptr(out), 0, 6, 4, ms, 1, ptr(cs), stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((cs == 9).all()), "n = 0 leaves the outputs alone"


def test_entry_point_refuses_device_pointers_too():
    """Every error-2 refusal of tests/test_crop_cpu.REFUSED with device buffers: the code comes back, nothing is launched, no buffer changes."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    frame, geom = torch.full((5 * 7 * 3,), 3, dtype=torch.uint8, device="cuda"), torch.full((4,), 5.0, device="cuda")
    out, cs, idx = torch.full((3 * 4 * 6,), 7.0, device="cuda"), torch.full((4,), 9.0, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(frames=ptr(frame), n_frames=1, Hf=5, Wf=7, row_stride=21, frame_stride=105, frame_index=None, geom=ptr(geom), kind=0, aspect=1.0, n=1, out=ptr(out),
             dtype=0, out_w=6, out_h=4, mean_std=MEAN + STD, swap=1, cs=ptr(cs)):
        m = None if mean_std is None else (C.c_float * 6)(*mean_std)
        return lib.kasf_crop_persons(frames, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, kind, aspect, n, out, dtype, out_w, out_h, m, swap, cs, stream())

    for kw in REFUSED:
        kw = {k: (ptr(idx) if v == "idx" else v) for k, v in kw.items()} if "frame_index" in kw else kw
        assert call(**kw) == 2 and lib.kasf_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((cs == 9).all()) and bool((frame == 3).all()) and bool((geom == 5).all())
    assert call(cs=None) == 0                                                    # center_scale_out is optional
    torch.cuda.synchronize()
    assert bool((cs == 9).all()) and not bool((out == 7).any())
