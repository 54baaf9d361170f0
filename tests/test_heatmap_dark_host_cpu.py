"""The DARK / UDP decode kernels of csrc/k_heatmap.hip without a GPU: the kernels' own source compiled for the host with g++ behind the lockstep emulation of
a workgroup (tests/host_emul/: one host thread per GPU thread, two barriers around every wave collective) and held to the numpy restatement of include/kasf.h's
rules (tests/test_heatmap_dark_cpu.py, heatmap_dark_decode_np), exactly.  It shows the kernels' logic -- which lane computes which horizontal sum, which lane
fetches which, the order of every sum, the fp64 step -- and their indexing (canaries around the outputs, inputs unchanged).  The emulation's shuffles need every
wave of a block to reach every collective alike, so each launch has a multiple of four maps (four persons: 68); ragged tails, bf16 and what only the device
can show stay with tests/test_gpu_heatmap_dark.py."""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build
from tests.test_heatmap_cpu import F32
from tests.test_heatmap_dark_cpu import gaussian_weights_np, heatmap_dark_decode_np, same_bits_nan
from tests.test_heatmap_flip_cpu import merge_np, partner_np

CANARY = 0x5A
N = 4                                                           # persons per launch: 68 maps, 17 whole workgroups
KERNELS = (1, 3, 11, 17)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "heatmap_dark_host", "emul_heatmap_dark.cpp")
    lib.emul_heatmap_decode.restype = None
    lib.emul_heatmap_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double,
                                        C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def behind_canaries(a):
    """A copy of `a` whose first byte is 16-byte aligned, 64 canary bytes on either side -> (whole uint8 buffer, view of the payload with a's dtype and shape)."""
    buf = np.full(a.nbytes + 160, CANARY, np.uint8)
    start = 64 + (-(buf.ctypes.data + 64) % 16)
    view = buf[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    view[...] = a
    return buf, view


def only_payload_changed(buf, view, before):
    now = buf.copy()
    off = view.ctypes.data - buf.ctypes.data
    now[off:off + view.nbytes] = before[off:off + view.nbytes]
    return np.array_equal(now, before)


def special_maps(H, W, dtype, seed):
    """[N,17,H,W]: every map a low random floor in (0, 0.3) with one peak on top; the first maps put it where the two stencils' bounds lie -- the corners, each
    edge, (1,1), (2,2), (H-3,W-3), (H-2,W-2) --, then an all-negative map, a constant positive one (its first maximum is the corner: no dark step, a zero
    gradient in dark_udp), one with a NaN, and a faint one -- 1e-12 at (2,2) over zeros, so that every blurred value falls under dark's 1e-10 clamp and
    det == 0 exactly (float32 only: the value is 0 in float16) --; the rest anywhere."""
    g = np.random.default_rng(seed)
    hm = g.uniform(0.0, 0.3, (N, 17, H, W))
    flat = hm.reshape(N * 17, H, W)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (1, 1), (2, 2), (H - 3, W - 3), (H - 2, W - 2)]
    spots = [(min(max(y, 0), H - 1), min(max(x, 0), W - 1)) for y, x in spots]
    for i in range(N * 17):
        y, x = spots[i] if i < len(spots) else (int(g.integers(0, H)), int(g.integers(0, W)))
        flat[i, y, x] += 1.0
        if x + 1 < W:
            flat[i, y, x + 1] += 0.6
        if y + 1 < H:
            flat[i, y + 1, x] += 0.4
    k = len(spots)
    flat[k] = -flat[k]
    flat[k + 1] = 0.25
    flat[k + 2, H // 2, W // 2] = np.nan
    flat[k + 3] = 0.0
    flat[k + 3, min(2, H - 1), min(2, W - 1)] = 1e-12
    return hm.astype(dtype)


def run(emul, hm, hmf, geom, kind, aspect, mode, kernel, udp, shift=True, partner=None, merged=False):
    H, W = hm.shape[-2:]
    dtype = 0 if hm.dtype == F32 else 2
    in_bufs = [behind_canaries(a) for a in ((hm, geom) if hmf is None else (hm, geom, hmf))]
    keep = [b.copy() for b, _ in in_bufs]
    out_buf, out = behind_canaries(np.full((N, 17, 3), -7.0, F32))
    mrg_buf, mrg = behind_canaries(np.full(hm.shape, -7.0, F32))
    before = out_buf.copy(), mrg_buf.copy()
    w = gaussian_weights_np(kernel) if mode else None
    table = None if partner is None else np.ascontiguousarray(partner, dtype=np.int32)
    launches = emul.emul_launches()
    emul.emul_heatmap_decode(in_bufs[0][1].ctypes.data, None if hmf is None else in_bufs[2][1].ctypes.data, dtype, N, H, W,
                             None if table is None else table.ctypes.data, int(shift), in_bufs[1][1].ctypes.data, kind, aspect, mode,
                             None if w is None else w.ctypes.data, kernel, int(udp), out.ctypes.data, mrg.ctypes.data if merged else None)
    assert emul.emul_launches() == launches + 1, "one launch"
    assert all(np.array_equal(b, k) for (b, _), k in zip(in_bufs, keep)), "inputs are only read"
    assert only_payload_changed(out_buf, out, before[0]) and (only_payload_changed(mrg_buf, mrg, before[1]) if merged else np.array_equal(mrg_buf, before[1]))
    return out.copy(), mrg.copy()


CASES = [((6, 8), np.float32), ((6, 8), np.float16), ((8, 12), np.float32), ((8, 12), np.float16), ((5, 3), np.float32), ((33, 31), np.float32)]


@pytest.mark.parametrize("si", range(len(CASES)), ids=[f"{h}x{w}-{np.dtype(d).name}" for (h, w), d in CASES])
def test_emulated_kernels_are_the_restatement(emul, si):
    """Vector path: 6 x 8 and 8 x 12 in fp32 and fp16 (flip-tested: ROW, ROW, ROW, SPLIT); element path: 5 x 3 and 33 x 31 (maps no multiple of 16 bytes).  Per
    shape: K in {1, 3, 11, 17} x {dark, dark_udp}, with flipped / udp / shift / boxes alternating so that every pairing occurs, and mode 0 with udp once."""
    (H, W), dtype = CASES[si]
    hm, hmf = special_maps(H, W, dtype, seed=si), special_maps(H, W, dtype, seed=100 + si)
    g = np.random.default_rng(si)
    cs = np.concatenate((g.uniform(50, 900, (N, 2)), g.uniform(0.5, 3.0, (N, 2))), axis=1).astype(F32)
    boxes = np.concatenate((g.uniform(0, 300, (N, 2)), g.uniform(400, 900, (N, 2))), axis=1).astype(F32)
    pairs = partner_np(((1, 2), (5, 6), (0, 16)))
    combos = [(ki, mi) for ki in range(4) for mi in range(2)] + [(0, -1)]
    seen = set()
    for ki, mi in combos:
        kernel, mode = KERNELS[ki], mi + 1
        flip, udp, shift, box = (ki + mi + si) % 2 == 0, (ki + si) % 2 == 0, (ki // 2 + mi) % 2 == 0, (ki + mi) % 2 == 1
        if mode == 0:
            kernel, flip, udp = 1, si % 2 == 0, True
        if udp and min(H, W) < 2:
            udp = False
        seen.add((mode, flip, udp))
        geo = dict(boxes=boxes, aspect=0.75) if box else dict(center=cs[:, :2], scale=cs[:, 2:])
        out, mrg = run(emul, hm, hmf if flip else None, boxes if box else cs, int(box), 0.75 if box else 1.0, mode, kernel, udp, shift,
                       (pairs if ki % 2 else partner_np()) if flip else None, merged=flip and mi == 0)     # the launcher takes a table; NULL is the entry point's
        raw = merge_np(hm, hmf, shift=shift, partner=pairs if ki % 2 else None) if flip else hm
        want, coords, dets = heatmap_dark_decode_np(raw, decode=("quarter", "dark", "dark_udp")[mode], kernel=kernel, udp=udp, parts=True, **geo)
        assert same_bits_nan(out, want), (kernel, mode, flip, udp, shift, box, np.argwhere(out.view(np.uint32) != want.view(np.uint32))[:4])
        if flip and mi == 0:
            assert same_bits_nan(mrg, raw)
        if mode == 1 and not flip and dtype == np.float32 and min(H, W) >= 6:
            assert dets.reshape(-1)[15] == 0 and coords.reshape(-1, 2)[15].tolist() == [2, 2], "the faint map: det == 0, no step"
    assert len(seen) >= 5


def test_the_special_maps_hold_what_they_claim():
    hm = special_maps(8, 12, np.float32, 0).reshape(-1, 8, 12)
    where = [np.unravel_index(np.argmax(m), m.shape) for m in hm[:12]]
    assert where[:4] == [(0, 0), (0, 11), (7, 0), (7, 11)] and where[8:] == [(1, 1), (2, 2), (5, 9), (6, 10)]
    assert hm[12].max() < 0 and (hm[13] == 0.25).all() and np.isnan(hm[14]).sum() == 1 and hm[15].max() == F32(1e-12)
    out, coords, dets = heatmap_dark_decode_np(hm[:17][None], np.zeros((1, 2), F32), np.ones((1, 2), F32), decode="dark", kernel=3, parts=True)
    assert dets[0, 15] == 0 and coords[0, 15].tolist() == [2, 2] and not coords[0, 12].any() and np.isnan(out[0, 14, 2]) and np.isnan(dets[0, 13])
    assert np.isnan(dets[0, :9]).all() and not np.isnan(dets[0, 9:11]).any() and np.isnan(dets[0, 11]), "dark steps at (2,2) and (H-3,W-3) only"
