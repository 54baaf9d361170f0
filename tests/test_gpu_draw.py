"""The overlay and the encoder's surface on the device (kasf_draw_poses / kasf_bgr_to_nv12 / kasf_pose_panel through K.draw_poses / bgr_to_nv12 /
poses_to_panel) against the numpy restatements of tests/test_draw_cpu.py, which that file ties to exact Fraction geometry and to the exact fp64 colour
conversion.  Device and restatement perform the same integer (panel: the same single fp32) operations, so every comparison is exact.  The case list is the one
tests/test_draw_host_cpu.py runs through the host-compiled kernel source.  Nothing here provokes a fault: refusals are tested through the error code in
tests/test_draw_cpu.py; no test looks at the kernel's assembly.

Placements (csrc/k_draw.hip chooses each stream's form by alignment): `grid` = views on torch's allocation grid behind pitches that are multiples of 8 (whole
blocks move as dwords), `odd` = slices one byte into their buffers behind odd pitches (bytes everywhere)."""
import itertools

import numpy as np
import pytest
import torch

from tests.test_draw_cpu import CASES, COMBOS, bgr_to_nv12_np, draw_poses_np, expected, noise_frames, pose_panel_np, skeletons
from tests.test_yuv_cpu import bounds as yuv_bounds, exact_coefficients as yuv_exact

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 0xEE, 0xC3
OUTPUTS = ("bgr", "surface", "both", "inplace", "inplace+surface")


def up(n, a):
    return (n + a - 1) // a * a


def pitched(shape, pitch, frame_stride, offset, fill, inner, data=None):
    """A device buffer of `fill` and the strided view [F,rows,cols,inner] into it, `offset` bytes past its start."""
    F, rows, cols = shape
    buf = torch.full((offset + (F - 1) * frame_stride + rows * pitch + 64,), fill, dtype=torch.uint8, device="cuda")
    view = buf[offset:].as_strided((F, rows, cols, inner), (frame_stride, pitch, inner, 1))
    if data is not None:
        view.copy_(torch.from_numpy(np.array(data)).reshape(F, rows, cols, inner))                  # (a copy: the shared cases are read-only)
    return buf, view


def only_payload_changed(buf, view, before):
    now, keep = buf.clone(), before.clone()
    for b in (now, keep):
        b[view.storage_offset():].as_strided(view.shape, view.stride()).zero_()
    return torch.equal(now, keep)


def run(case, where="grid", outputs="both", matrix="bt601", full_range=False, rgb=False, batched=True):
    """K.draw_poses on pitched device views -> (frame, y, uv) as numpy, or None; asserts that inputs and every padding byte survive."""
    import kasportsformer_amd as K
    frames, kp, valid, kw = case["frames"], case["kp"], case["valid"], dict(case["kw"])
    F, Hf, Wf = frames.shape[:3]
    ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
    if where == "odd":
        off, fp, op, yp, cp = 1, 3 * Wf + 7, 3 * Wf + 5, Wf + 3, 2 * cw + 3
        ff, of, yf, cf = Hf * fp + 5, Hf * op + 3, Hf * yp + 7, ch * cp + 5
    else:
        off, fp, op, yp, cp = 0, up(3 * Wf, 8) + 8, up(3 * Wf, 8) + 16, up(Wf, 8) + 8, up(2 * cw, 8) + 8
        ff, of, yf, cf = Hf * fp + 16, Hf * op + 24, Hf * yp + 16, ch * cp + 8
    sbuf, src = pitched((F, Hf, Wf), fp, ff, off, PAD, 3, frames)
    in_place = outputs.startswith("inplace")
    obuf, out = (sbuf, src) if in_place else (pitched((F, Hf, Wf), op, of, off, SENTINEL, 3) if outputs in ("bgr", "both") else (None, None))
    surface = outputs in ("surface", "both", "inplace+surface")
    ybuf, y = pitched((F, Hf, Wf), yp, yf, off, SENTINEL, 1) if surface else (None, None)
    uvbuf, uv = pitched((F, ch, cw), cp, cf, off, SENTINEL, 2) if surface else (None, None)
    before = {id(b): b.clone() for b in (sbuf, obuf, ybuf, uvbuf) if b is not None}
    kpt = None if kp is None else torch.from_numpy(np.array(kp)).cuda()
    vt = None if valid is None else torch.from_numpy(np.array(valid)).cuda()
    pick = (lambda t: None if t is None else (t if batched else t[0]))
    res = K.draw_poses(pick(src), pick(kpt), pick(vt), out=pick(out) if out is not None else False, surface=(pick(y[..., 0]), pick(uv)) if surface else False,
                       matrix=matrix, full_range=full_range, rgb=rgb, **kw)
    torch.cuda.synchronize()
    assert (res.frame is None) == (out is None) and (res.y is None) == (not surface)
    if in_place:
        assert res.frame.data_ptr() == src.data_ptr()
        assert only_payload_changed(sbuf, src, before[id(sbuf)]), "in place only the frame's payload changes"
    else:
        assert torch.equal(sbuf, before[id(sbuf)]), "the frame is only read"
    for b, v in ((obuf, out), (ybuf, y), (uvbuf, uv)):
        assert b is None or only_payload_changed(b, v, before[id(b)]), "padding survives"
    if kpt is not None:
        assert torch.equal(kpt.cpu(), torch.from_numpy(np.array(kp))) or np.isnan(kp).any()
    return (None if out is None else out.cpu().numpy(), None if y is None else y[..., 0].cpu().numpy(), None if uv is None else uv.cpu().numpy())


def check(got, painted, combo, what):
    frame, y, uv = got
    if frame is not None:
        assert np.array_equal(frame, painted), (what, "frame")
    if y is not None:
        wy, wuv = bgr_to_nv12_np(painted, *combo)
        assert np.array_equal(y, wy), (what, combo, "luma")
        assert np.array_equal(uv, wuv), (what, combo, "chroma")


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_restatement(name):
    """The host test's case list at the same shapes: every placement x output set, tables and rgb rotating."""
    case, painted = expected(name)
    combos = itertools.cycle(COMBOS)
    for where, outputs in itertools.product(("grid", "odd"), OUTPUTS):
        combo = next(combos)
        check(run(case, where, outputs, *combo), painted, combo, (name, where, outputs))


def test_same_bits_on_a_second_run_alone_and_in_a_batch_of_three():
    case, painted = expected("odd")
    three = dict(frames=case["frames"][[0, 1, 0]], kp=case["kp"][[0, 1, 1]], valid=case["valid"][[0, 1, 1]], kw=case["kw"])
    first, second = run(three, "grid", "both"), run(three, "grid", "both")
    for a, b in zip(first, second):
        assert np.array_equal(a, b), "the same bits from run to run"
    for f in range(3):
        one = {k: (v[f:f + 1] if k != "kw" else v) for k, v in three.items()}
        for batched in (True, False):
            alone = run(one, "odd", "both", batched=batched)
            for a, b in zip(alone, first):
                assert np.array_equal(a[0], b[f]), (f, batched)
    check(tuple(a[:2] for a in first), painted, COMBOS[0], "batch of three")
    want = draw_poses_np(three["frames"][2:], three["kp"][2:], three["valid"][2:], **case["kw"])
    assert np.array_equal(first[0][2], want[0])


def test_strided_keypoints_a_tracked_ticks_valid_and_one_launch_per_call(monkeypatch):
    """keypoints as the x, y view of a wider tensor (no copy: the entry point gets the view's own address and strides), valid as TrackedTick's bool [B, R]; a spy
    on the library symbols sees one launch per call."""
    import kasportsformer_amd as K
    from kasportsformer_amd import _lib
    lib = _lib.load()
    seen = []
    for sym in ("kasf_draw_poses", "kasf_bgr_to_nv12", "kasf_pose_panel"):
        real = getattr(lib, sym)
        monkeypatch.setattr(lib, sym, (lambda real, sym: lambda *a: (seen.append((sym, a)), real(*a))[1])(real, sym))
    F, P, Hf, Wf = 2, 4, 50, 140
    frames = noise_frames(F, Hf, Wf, 21)
    wide = np.zeros((F, P, 17, 5), np.float32)
    wide[..., 1:4] = skeletons(F, P, Hf, Wf, 22)
    valid = np.array([[True, False, True, True], [True, True, False, True]])
    wt = torch.from_numpy(wide).cuda()
    fr = torch.from_numpy(frames).cuda()
    kp = wt[..., 1:3]
    res = K.draw_poses(fr, kp, torch.from_numpy(valid).cuda(), surface=True)
    assert len(seen) == 1 and seen[0][0] == "kasf_draw_poses"
    a = seen[0][1]
    assert a[0] == fr.data_ptr() and a[6] == kp.data_ptr() and tuple(a[7:14]) == (P, 17, 2, P * 17 * 5, 17 * 5, 5, 1), "read in place through its strides"
    want = draw_poses_np(frames, wide[..., 1:3], valid, colors=K.draw.hue_wheel(16))
    assert np.array_equal(res.frame.cpu().numpy(), want) and res.frame.data_ptr() != fr.data_ptr()
    wy, wuv = bgr_to_nv12_np(want)
    assert np.array_equal(res.y.cpu().numpy(), wy) and np.array_equal(res.uv.cpu().numpy(), wuv)
    assert torch.equal(fr.cpu(), torch.from_numpy(frames)), "without out= the frame is not touched"
    # scores: the x, y, score view, and numpy input
    res3 = K.draw_poses(frames, wide[..., 1:4], valid, min_score=0.5, thickness=3, dot_radius=0)
    want3 = draw_poses_np(frames, wide[..., 1:4], valid, colors=K.draw.hue_wheel(16), min_score=0.5, thickness=3, dot_radius=0)
    assert np.array_equal(res3.frame.cpu().numpy(), want3) and res3.y is None and len(seen) == 2
    # in place, unbatched
    one = fr[0].clone()
    r = K.draw_poses(one, kp[0], out=one)
    assert r.frame is one and np.array_equal(one.cpu().numpy(), draw_poses_np(frames[:1], wide[:1, ..., 1:3], None, colors=K.draw.hue_wheel(16))[0]) and len(seen) == 3
    y, uv = K.bgr_to_nv12(fr)
    assert len(seen) == 4 and seen[3][0] == "kasf_bgr_to_nv12"
    wy, wuv = bgr_to_nv12_np(frames)
    assert np.array_equal(y.cpu().numpy(), wy) and np.array_equal(uv.cpu().numpy(), wuv)


@pytest.mark.parametrize("Hf,Wf", [(1, 1), (2, 2), (3, 5), (7, 8), (37, 23), (33, 130), (64, 256)])
def test_bgr_to_nv12_equals_the_restatement(Hf, Wf):
    import kasportsformer_amd as K
    combos = itertools.cycle(COMBOS)
    for F in (1, 3):
        fr = noise_frames(F, Hf, Wf, 100 * Hf + Wf)
        for where in ("grid", "odd"):
            matrix, full_range, rgb = next(combos)
            ch, cw = (Hf + 1) // 2, (Wf + 1) // 2
            off, fp, yp, cp = (1, 3 * Wf + 7, Wf + 3, 2 * cw + 3) if where == "odd" else (0, up(3 * Wf, 8) + 8, up(Wf, 8) + 8, up(2 * cw, 8) + 8)
            sbuf, src = pitched((F, Hf, Wf), fp, Hf * fp + 16, off, PAD, 3, fr)
            ybuf, y = pitched((F, Hf, Wf), yp, Hf * yp + 16, off, SENTINEL, 1)
            uvbuf, uv = pitched((F, ch, cw), cp, ch * cp + 8, off, SENTINEL, 2)
            before = [b.clone() for b in (sbuf, ybuf, uvbuf)]
            got = K.bgr_to_nv12(src, surface=(y[..., 0], uv), matrix=matrix, full_range=full_range, rgb=rgb)
            assert got[0].data_ptr() == y.data_ptr() and got[1].data_ptr() == uv.data_ptr()
            wy, wuv = bgr_to_nv12_np(fr, matrix, full_range, rgb)
            assert np.array_equal(y[..., 0].cpu().numpy(), wy) and np.array_equal(uv.cpu().numpy(), wuv), (F, where, matrix, full_range, rgb)
            assert torch.equal(sbuf, before[0]) and only_payload_changed(ybuf, y, before[1]) and only_payload_changed(uvbuf, uv, before[2])
        y, uv = K.bgr_to_nv12(fr[0])
        wy, wuv = bgr_to_nv12_np(fr[0])
        assert np.array_equal(y.cpu().numpy(), wy) and np.array_equal(uv.cpu().numpy(), wuv)


def round_trip_limit(matrix, full_range):
    """The round trip's bound per channel, {"B", "G", "R"} -> grey levels, from the two stated accuracies (the derivation is in the test below; the composed
    tick tests import it from here)."""
    from tests.test_draw_cpu import nv12_bound
    bY, bU, bV = nv12_bound(matrix, full_range)
    _, (iB, iG, iR) = yuv_bounds(matrix, full_range)
    cy, cvr, cvg, cug, cub = yuv_exact(matrix, full_range)
    return {"B": iB + cy * bY + abs(cub) * bU, "G": iG + cy * bY + abs(cug) * bU + abs(cvg) * bV, "R": iR + cy * bY + abs(cvr) * bV}


@pytest.mark.parametrize("matrix,full_range", [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)])
def test_a_flat_colour_survives_the_round_trip_within_the_two_bounds(matrix, full_range):
    """yuv_to_bgr(bgr_to_nv12(frame)) on flat-colour frames.  Each of Y, U, V is within its stated bound b_f (tests/test_draw_cpu.py, nv12_bound: 0.5 + ...) of
    the exact conversion of the colour -- the quad's mean IS the colour --; the exact inverse maps those errors into a channel with its coefficients (clamps are
    1-Lipschitz), and yuv_to_bgr's own stated bound b_i (tests/test_yuv_cpu.py, bounds) comes on top: |error| <= b_i + |cy| bY + sum |c| b_chroma, an integer, so
    at most its floor.  That is 2 grey levels for every table; it is computed here, not assumed."""
    import kasportsformer_amd as K
    limit = round_trip_limit(matrix, full_range)
    print(matrix, full_range, limit)
    assert max(int(v) for v in limit.values()) <= 2, "the two grey levels the round trip is stated to keep"
    g = np.random.default_rng(1)
    colours = np.concatenate([np.array(list(itertools.product((0, 255), repeat=3))), np.stack([np.arange(0, 256, 17)] * 3, axis=1), g.integers(0, 256, size=(40, 3))])
    frames = np.broadcast_to(colours[:, None, None, :].astype(np.uint8), (len(colours), 6, 10, 3)).copy()
    y, uv = K.bgr_to_nv12(frames, matrix=matrix, full_range=full_range)
    back = K.yuv_to_bgr(y, uv, matrix=matrix, full_range=full_range).cpu().numpy().astype(int)
    err = np.abs(back - frames.astype(int)).max(axis=(0, 1, 2))
    print("worst B, G, R:", err)
    for c, name in enumerate("BGR"):
        assert err[c] <= int(limit[name]), (name, err)


def test_the_panel_is_projected_and_drawn():
    import kasportsformer_amd as K
    g = np.random.default_rng(8)
    world = g.normal(0.0, 0.3, size=(2, 3, 17, 3)).astype(np.float32)
    rect = (70, 2, 138, 48)
    view = K.draw.panel_view(rect, 15.0, 70.0)
    got = K.poses_to_panel(torch.from_numpy(world).cuda(), rect, 15.0, 70.0)
    want = pose_panel_np(world, view)
    assert got.shape == (2, 3, 17, 2) and np.array_equal(got.cpu().numpy(), want), "the same single fp32 operations: the same bits"
    assert np.array_equal(K.poses_to_panel(world[0, 0], rect, 15.0, 70.0).cpu().numpy(), want[0, 0])
    big = g.normal(0.0, 0.3, size=(700, 17, 3)).astype(np.float32)                        # more than one block
    assert np.array_equal(K.poses_to_panel(big, rect).cpu().numpy(), pose_panel_np(big, K.draw.panel_view(rect)))
    frames = noise_frames(2, 50, 140, 9)
    fills = [[rect[0], rect[1], rect[2], rect[3], 255, 255, 255]]
    res = K.draw_poses(frames, got, fills=fills, thickness=1, dot_radius=1)
    assert np.array_equal(res.frame.cpu().numpy(), draw_poses_np(frames, want, None, colors=K.draw.hue_wheel(16), fills=fills, thickness=1, dot_radius=1))
