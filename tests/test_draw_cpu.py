"""The overlay and the encoder's surface (kasf_draw_poses / kasf_bgr_to_nv12 / kasf_pose_panel, K.draw_poses / bgr_to_nv12 / poses_to_panel) without a GPU:
`draw_poses_np`, `bgr_to_nv12_np` and `pose_panel_np`, the numpy restatements of include/kasf.h's rules that the host-emulation and GPU tests hold the kernels to
bit for bit, the case list those two files share, and what ties the restatements themselves down:

  coverage    on small frames, with fractions.Fraction geometry: a pixel is covered iff its exact distance to the closed segment is <= t / 2 (to the dot's centre
              <= r); dots are symmetric; the int64 form with the guard equals the rule in unbounded Python integers, also for far-away endpoints.
  order       a later person's line over an earlier person's dot; fills first.
  visibility  int(-0.5) == 0; NaN / inf / out-of-bounds joints, a score <= min_score, a NaN score, a row with valid == 0.
  tables      the header's literals re-derived from Kr, Kb; luma over all 2^24 (B, G, R) and chroma over all 2^24 uniform quads and 10^6 random quads within
              0.5 + sum |c_int / 2^20 - c| * 255 of the exact fp64 conversion -- the bound is computed from the tables, not measured.
  panel       against an fp64 projection, to a few fp32 ulps of the panel size.
  refusals    every error-2 condition of the three C entry points (which touch no pointer), and the Python argument checks that need no device.

NOT verified here or anywhere: equality with cv2.line / cv2.circle (this is exact geometry, not OpenCV's rasteriser) or with an encoder's colour handling."""
import ctypes as C
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rule 5: { CRY, CGY, CBY, CRU, CGU, CH, CGV, CBV } per (matrix, full_range); CBU = CRV = CH
TABLES = {
    ("bt601", False): (269262, 528618, 102662, -155423, -305128, 460551, -385654, -74897),
    ("bt601", True): (313524, 615514, 119538, -176932, -347356, 524288, -439026, -85262),
    ("bt709", False): (191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230),
    ("bt709", True): (222927, 749942, 75707, -120138, -404150, 524288, -476214, -48074),
}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
H36M_SEGMENTS = tuple(zip((0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15), range(1, 17)))
TILE_W, TILE_H, LIST = 128, 32, 256                # csrc/k_draw.hip's tile and list; tests/test_draw_host_cpu.py checks them against the kernel's constants


# ---- the restatement: geometry ----
def joint_pixel(x, y, score=None, min_score=None):
    """Rule 1 without `valid`: (xi, yi) or None."""
    if not (math.isfinite(x) and math.isfinite(y)):
        return None
    xi, yi = int(x), int(y)
    if not (-32768 <= xi <= 65535 and -32768 <= yi <= 65535):
        return None
    if score is not None and min_score is not None and math.isfinite(min_score) and not score > min_score:
        return None
    return xi, yi


def line_cover(X, Y, A, B, t):
    """Rule 3 on int64 pixel grids, with the guard that keeps 4 c^2 inside int64."""
    dx, dy = np.int64(B[0] - A[0]), np.int64(B[1] - A[1])
    wx, wy = X - np.int64(A[0]), Y - np.int64(A[1])
    L2, s, c = dx * dx + dy * dy, wx * dx + wy * dy, wx * dy - wy * dx
    t2 = np.int64(t * t)
    at_a = 4 * (wx * wx + wy * wy) <= t2
    ux, uy = wx - dx, wy - dy
    at_b = 4 * (ux * ux + uy * uy) <= t2
    ac = np.abs(c)
    far = 2 * ac > np.int64(t) * (abs(dx) + abs(dy))
    ac = np.where(far, 0, ac)
    between = ~far & (4 * ac * ac <= t2 * L2)
    return np.where((L2 == 0) | (s <= 0), at_a, np.where(s >= L2, at_b, between))


def line_cover_exact(px, py, A, B, t):
    """Rule 3 for one pixel in Python's unbounded integers, as it is written (no guard)."""
    dx, dy, wx, wy = B[0] - A[0], B[1] - A[1], px - A[0], py - A[1]
    L2, s, c = dx * dx + dy * dy, wx * dx + wy * dy, wx * dy - wy * dx
    if L2 == 0 or s <= 0:
        return 4 * (wx * wx + wy * wy) <= t * t
    if s >= L2:
        return 4 * ((wx - dx) ** 2 + (wy - dy) ** 2) <= t * t
    return 4 * c * c <= t * t * L2


def draw_poses_np(frames, keypoints=None, valid=None, segments=H36M_SEGMENTS, colors=None, dot_color=(255, 255, 255), thickness=2, dot_radius=2, min_score=None,
                  fills=None, boxed=False):
    """The numpy restatement of rules 1-4: frames uint8 [F,Hf,Wf,3], keypoints [F,P,J,C], valid [F,P] -> the painted frames.  Primitives are painted in rule
    2's order, later ones over earlier ones, each evaluated over the whole frame -- or, with `boxed` (what a host implementation would do at 1080p;
    tools/draw_bench.py), over the primitive's box grown by ceil(t / 2) or r, outside which rule 3 cannot hold; the tests show both give the same frames."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    F, Hf, Wf = out.shape[:3]
    segments = np.asarray(segments, np.int64).reshape(-1, 2)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3) if colors is not None else None
    dot = np.asarray(dot_color, np.uint8)

    def window(lo_x, lo_y, hi_x, hi_y):
        """The frame, or its part inside the inclusive box: (slices, X, Y)."""
        x0, y0, x1, y1 = (max(lo_x, 0), max(lo_y, 0), min(hi_x + 1, Wf), min(hi_y + 1, Hf)) if boxed else (0, 0, Wf, Hf)
        Y, X = np.meshgrid(np.arange(y0, max(y1, y0), dtype=np.int64), np.arange(x0, max(x1, x0), dtype=np.int64), indexing="ij")
        return (slice(y0, max(y1, y0)), slice(x0, max(x1, x0))), X, Y

    h = (thickness + 1) // 2
    for f in range(F):
        for q in ([] if fills is None else np.asarray(fills, np.int64).reshape(-1, 7)):
            x0, y0, x1, y1 = max(int(q[0]), 0), max(int(q[1]), 0), min(int(q[2]), Wf), min(int(q[3]), Hf)
            if x0 < x1 and y0 < y1:
                out[f, y0:y1, x0:x1] = (q[4:7] & 255).astype(np.uint8)
        if keypoints is None:
            continue
        kp = np.asarray(keypoints)[f]
        P, J, Cc = kp.shape
        for p in range(P):
            if valid is not None and not np.asarray(valid)[f, p]:
                continue
            pix = [joint_pixel(float(kp[p, j, 0]), float(kp[p, j, 1]), float(kp[p, j, 2]) if Cc == 3 else None, min_score) for j in range(J)]
            for s, (ja, jb) in enumerate(segments):
                A = pix[ja] if 0 <= ja < J else None
                B = pix[jb] if 0 <= jb < J else None
                if A is not None and B is not None:
                    w, X, Y = window(min(A[0], B[0]) - h, min(A[1], B[1]) - h, max(A[0], B[0]) + h, max(A[1], B[1]) + h)
                    out[f][w][line_cover(X, Y, A, B, thickness)] = colors[s]
                for D in (A, B):
                    if D is not None:
                        w, X, Y = window(D[0] - dot_radius, D[1] - dot_radius, D[0] + dot_radius, D[1] + dot_radius)
                        out[f][w][(X - D[0]) ** 2 + (Y - D[1]) ** 2 <= dot_radius * dot_radius] = dot
    return out


# ---- the restatement: the surface ----
def bgr_to_nv12_np(frames, matrix="bt601", full_range=False, rgb=False):
    """Rule 5: uint8 [F,Hf,Wf,3] (or [Hf,Wf,3]) -> (y [..,Hf,Wf], uv [..,ch,cw,2]) uint8, in int32 throughout."""
    fr = np.asarray(frames)
    single = fr.ndim == 3
    fr = (fr[None] if single else fr).astype(np.int32)
    cry, cgy, cby, cru, cgu, chh, cgv, cbv = (np.int32(c) for c in TABLES[(matrix, bool(full_range))])
    R, G, B = (fr[..., 0], fr[..., 1], fr[..., 2]) if rgb else (fr[..., 2], fr[..., 1], fr[..., 0])
    yoff = np.int32(0 if full_range else 16)
    y = np.clip((cry * R + cgy * G + cby * B + (yoff << 20) + (1 << 19)) >> 20, 0, 255).astype(np.uint8)
    F, Hf, Wf = R.shape
    yy, xx = np.minimum(np.arange(2 * ((Hf + 1) // 2)), Hf - 1), np.minimum(np.arange(2 * ((Wf + 1) // 2)), Wf - 1)         # the last row / column again at an odd edge
    sums = [c[:, yy][:, :, xx].reshape(F, (Hf + 1) // 2, 2, (Wf + 1) // 2, 2).sum(axis=(2, 4), dtype=np.int32) for c in (R, G, B)]
    u = np.clip((cru * sums[0] + cgu * sums[1] + chh * sums[2] + (128 << 22) + (1 << 21)) >> 22, 0, 255)
    v = np.clip((chh * sums[0] + cgv * sums[1] + cbv * sums[2] + (128 << 22) + (1 << 21)) >> 22, 0, 255)
    uv = np.stack((u, v), axis=-1).astype(np.uint8)
    return (y[0], uv[0]) if single else (y, uv)


def exact_coefficients(matrix, full_range):
    """The eight exact doubles of rule 5 from Kr, Kb, the luma scale and the chroma scale."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    ls, cs = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    return (kr * ls, kg * ls, kb * ls, -kr * cs / (2 * (1 - kb)), -kg * cs / (2 * (1 - kb)), cs / 2, -kg * cs / (2 * (1 - kr)), -kb * cs / (2 * (1 - kr)))


def nv12_bound(matrix, full_range):
    """0.5 + sum |c_int / 2^20 - c| * 255, per output channel (Y, U, V): every operand (a sample, or a quad's mean) is at most 255."""
    d = [abs(ci / 2.0 ** 20 - ce) * 255.0 for ci, ce in zip(TABLES[(matrix, full_range)], exact_coefficients(matrix, full_range))]
    return 0.5 + d[0] + d[1] + d[2], 0.5 + d[3] + d[4] + d[5], 0.5 + d[5] + d[6] + d[7]


# ---- the restatement: the panel ----
def pose_panel_np(world, view):
    """kasf_pose_panel in numpy fp32, one rounding per operation in the header's order: world [...,17,3] -> [...,17,2]."""
    w = np.asarray(world, np.float32)
    v = np.asarray(view, np.float32)
    d = w - w[..., :1, :]
    x = ((v[0] * d[..., 0] + v[1] * d[..., 1]) + v[2] * d[..., 2]) + v[6]
    y = ((v[3] * d[..., 0] + v[4] * d[..., 1]) + v[5] * d[..., 2]) + v[7]
    return np.stack((x, y), axis=-1).astype(np.float32)


# ---- the cases tests/test_draw_host_cpu.py and tests/test_gpu_draw.py share ----
def noise_frames(F, Hf, Wf, seed):
    g = np.random.default_rng(seed)
    fr = g.integers(0, 256, size=(F, Hf, Wf, 3), dtype=np.uint8)
    fr[:, 0, 0], fr[:, -1, -1] = 255, 0
    return fr


def skeletons(F, P, Hf, Wf, seed, C=3, spread=0.5):
    """[F,P,17,C] fp32: P random 17-joint figures per frame around random centres, fractional coordinates, scores in (0, 1)."""
    g = np.random.default_rng(seed)
    centre = g.uniform((0, 0), (Wf, Hf), size=(F, P, 1, 2))
    kp = centre + g.normal(0.0, spread * min(Hf, Wf) / 2 + 2, size=(F, P, 17, 2))
    if C == 3:
        kp = np.concatenate([kp, g.uniform(0.05, 1.0, size=(F, P, 17, 1))], axis=-1)
    return kp.astype(np.float32)


def wheel(n):
    from kasportsformer_amd.draw import hue_wheel
    return hue_wheel(n)


def make_case(name):
    """-> dict(frames [F,Hf,Wf,3] uint8, kp [F,P,J,C] fp32 or None, valid [F,P] uint8 or None, kw = the drawing arguments of draw_poses_np)."""
    seg16 = dict(segments=np.asarray(H36M_SEGMENTS, np.int32), colors=wheel(16))
    if name.startswith("tiny"):                                  # 1 x 1, 1 x 7, 2 x 2: less than a block, less than a quad
        Hf, Wf = {"tiny1x1": (1, 1), "tiny1x7": (1, 7), "tiny2x2": (2, 2)}[name]
        kp = np.zeros((1, 1, 3, 2), np.float32)
        kp[0, 0] = [(-3.5, -2.5), (Wf - 0.5, Hf - 0.5), (Wf + 40.0, 0.0)]
        return dict(frames=noise_frames(1, Hf, Wf, 1), kp=kp, valid=None,
                    kw=dict(segments=np.array([[0, 1], [1, 2]], np.int32), colors=wheel(2), dot_color=(1, 2, 3), thickness=1, dot_radius=0))
    if name == "odd":                                            # 3 x 3 tiles, F = 2 with different figures, P = 3, scores and a dropped row
        F, P, Hf, Wf = 2, 3, 67, 259
        valid = np.array([[1, 1, 0], [1, 1, 1]], np.uint8)
        return dict(frames=noise_frames(F, Hf, Wf, 2), kp=skeletons(F, P, Hf, Wf, 3), valid=valid,
                    kw=dict(**seg16, dot_color=(250, 251, 252), thickness=2, dot_radius=2, min_score=0.3,
                            fills=np.array([[200, -5, 300, 20, 9, 8, 7], [210, 10, 250, 90, 300, 1, 2], [-4, 60, 3, 64, 5, 5, 5], [50, 50, 50, 60, 1, 1, 1]], np.int32)))
    if name == "empty":                                          # P = 0: fills alone, two tiles
        return dict(frames=noise_frames(1, 35, 130, 4), kp=np.zeros((1, 0, 17, 2), np.float32), valid=None,
                    kw=dict(**seg16, fills=np.array([[100, 20, 131, 40, 0, 255, 0]], np.int32)))
    if name == "chunked":                                        # every bone of every person through one point: 14 * 48 primitives in one tile's list of 256
        F, P, Hf, Wf = 1, 14, 34, 131
        kp = skeletons(F, P, Hf, Wf, 5, C=2, spread=0.2)
        kp[:, :, 0] = (40.25, 13.75)                             # the root, on bones 0, 3 and 6
        kp[:, :, 8] = (41.0, 14.5)                               # the thorax, on bones 7, 8, 10 and 13
        kp[:, :, 1::2] = (40.9, 13.1)                            # ... so that every bone has an end within two pixels of (40, 13)
        kp[:, 1::2, 0, 0] += 3.0
        return dict(frames=noise_frames(F, Hf, Wf, 6), kp=kp, valid=None, kw=dict(**seg16, dot_color=(7, 7, 7), thickness=2, dot_radius=1))
    if name == "edge":                                           # degenerate, outside, far away, not finite, out of bounds; int(-0.5) == 0
        Hf, Wf = 37, 53
        kp = np.zeros((1, 3, 10, 2), np.float32)
        kp[0, 0] = [(10.2, 10.9), (10.7, 10.1), (-200.0, -100.0), (-90.0, -300.0), (-30000.0, -20000.0), (60000.0, 50000.0), (-0.5, -0.5), (4.0, 30.0),
                    (-30000.0, -20000.0), (60030.0, 40040.0)]                                  # 4 -> 5 passes 3,333 rows below the frame, 8 -> 9 through it
        kp[0, 1] = [(np.nan, 5.0), (20.0, 20.0), (np.inf, 3.0), (25.0, 25.0), (-32769.0, 10.0), (30.0, 12.0), (65536.5, 10.0), (30.0, 15.0), (2.0, 2.0), (2.0, -np.inf)]
        kp[0, 2] = [(-32768.9, 30.0), (65535.9, 33.0), (45.0, -32768.5), (47.0, 65535.5), (52.9, 36.9), (52.0, 36.0), (1e30, 1e30), (-1e30, 5.0), (0.0, 36.0), (9.0, 36.9)]
        return dict(frames=noise_frames(1, Hf, Wf, 7), kp=kp, valid=None,
                    kw=dict(segments=np.array([[0, 1], [2, 3], [4, 5], [6, 7], [1, 1], [8, 9]], np.int32), colors=wheel(6), dot_color=(0, 0, 0), thickness=3,
                            dot_radius=1))
    if name.startswith("t"):                                     # t in {1, 2, 7, 64} x r in {0, 2, 32}
        t, r = (int(v) for v in name[1:].split("r"))
        F, P, Hf, Wf = 1, 2, 45, 150
        return dict(frames=noise_frames(F, Hf, Wf, 8), kp=skeletons(F, P, Hf, Wf, 9 + t, C=2), valid=None,
                    kw=dict(**seg16, dot_color=(255, 0, 255), thickness=t, dot_radius=r))
    raise KeyError(name)


CASES = ("tiny1x1", "tiny1x7", "tiny2x2", "odd", "empty", "chunked", "edge", "t1r0", "t2r2", "t7r32", "t64r2")
COMBOS = [(m, fr, rgb) for (m, fr) in sorted(TABLES) for rgb in (False, True)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(case, painted frames) -- computed once, shared, read-only."""
    case = make_case(name)
    painted = draw_poses_np(case["frames"], case["kp"], case["valid"], **case["kw"])
    for a in (case["frames"], case["kp"], painted):
        if a is not None:
            a.flags.writeable = False
    return case, painted


@pytest.mark.parametrize("name", ["odd", "edge", "t64r2", "t7r32"])
def test_boxed_evaluation_changes_nothing(name):
    case, painted = expected(name)
    assert np.array_equal(draw_poses_np(case["frames"], case["kp"], case["valid"], boxed=True, **case["kw"]), painted)
    assert not np.array_equal(painted, case["frames"])


def primitives_through_tile(case, tx, ty):
    """How many drawn primitives' bounding boxes (as csrc/k_draw.hip grows them) meet tile (tx, ty) of frame 0."""
    kw, kp = case["kw"], case["kp"][0]
    Hf, Wf = case["frames"].shape[1:3]
    x0, y0, x1, y1 = tx * TILE_W, ty * TILE_H, min((tx + 1) * TILE_W, Wf), min((ty + 1) * TILE_H, Hf)
    h, r, n = (kw["thickness"] + 1) // 2, kw["dot_radius"], 0
    for p in range(kp.shape[0]):
        for ja, jb in kw["segments"]:
            A, B = joint_pixel(*map(float, kp[p, ja, :2])), joint_pixel(*map(float, kp[p, jb, :2]))
            if A and B:
                n += min(A[0], B[0]) - h < x1 and max(A[0], B[0]) + h >= x0 and min(A[1], B[1]) - h < y1 and max(A[1], B[1]) + h >= y0
            for D in (A, B):
                if D:
                    n += D[0] - r < x1 and D[0] + r >= x0 and D[1] - r < y1 and D[1] + r >= y0
    return n


def test_the_chunked_case_overflows_one_list_twice_over():
    case, _ = expected("chunked")
    n = primitives_through_tile(case, 0, 0)
    print("primitives through tile (0, 0):", n)
    assert n > 2 * LIST


# ---- coverage ----
def seg_dist2(px, py, A, B):
    """The exact squared distance from the pixel to the closed segment."""
    dx, dy = B[0] - A[0], B[1] - A[1]
    L2 = dx * dx + dy * dy
    u = Fraction(0) if L2 == 0 else min(Fraction(1), max(Fraction(0), Fraction((px - A[0]) * dx + (py - A[1]) * dy, L2)))
    cx, cy = A[0] + u * dx, A[1] + u * dy
    return (px - cx) ** 2 + (py - cy) ** 2


@pytest.mark.parametrize("t", [1, 2, 3, 7, 64])
def test_line_coverage_is_the_exact_distance_to_the_segment(t):
    Hf, Wf = 23, 29
    Y, X = np.meshgrid(np.arange(Hf, dtype=np.int64), np.arange(Wf, dtype=np.int64), indexing="ij")
    g = np.random.default_rng(t)
    ends = [((3, 4), (20, 17)), ((5, 5), (5, 5)), ((0, 11), (28, 11)), ((14, -3), (14, 30)), ((-10, -10), (40, 35)), ((27, 2), (1, 21))]
    ends += [(tuple(g.integers(-8, 36, 2)), tuple(g.integers(-8, 36, 2))) for _ in range(6)]
    for A, B in ends:
        A, B = tuple(int(v) for v in A), tuple(int(v) for v in B)
        got = line_cover(X, Y, A, B, t)
        for py in range(Hf):
            for px in range(Wf):
                inside = seg_dist2(px, py, A, B) <= Fraction(t * t, 4)
                assert bool(got[py, px]) == inside == line_cover_exact(px, py, A, B, t), (A, B, t, px, py)


def test_far_endpoints_stay_exact_in_int64():
    """The segment of the case list from (-30000, -20000) to (60000, 50000), and the extremes of rule 1: the guarded int64 form equals the rule in Python
    integers at every pixel of a frame's four corners' neighbourhoods, where |c| is largest."""
    for A, B in (((-30000, -20000), (60000, 50000)), ((-32768, -32768), (65535, 65535)), ((-32768, 65535), (65535, -32768)), ((65535, 0), (-32768, 1))):
        for (ox, oy) in ((0, 0), (32700, 0), (0, 32700), (32700, 32700), (16000, 15800)):
            Y, X = np.meshgrid(np.arange(oy, oy + 67, dtype=np.int64), np.arange(ox, ox + 67, dtype=np.int64), indexing="ij")
            for t in (1, 64):
                got = line_cover(X, Y, A, B, t)
                want = np.array([[line_cover_exact(int(x), int(y), A, B, t) for x in X[0]] for y in Y[:, 0]])
                assert np.array_equal(got, want), (A, B, ox, oy, t)
    # the bounds kasf.h states: 4 c^2 after the guard, and t^2 L2, stay inside int64
    assert 4 * (64 * 196606 // 2) ** 2 < 2 ** 48 and 64 * 64 * 2 * 98303 ** 2 < 2 ** 47 < 2 ** 63


@pytest.mark.parametrize("r", [0, 1, 2, 5, 32])
def test_dots_are_symmetric_discs(r):
    fr = np.zeros((1, 71, 71, 3), np.uint8)
    kp = np.array([[[[35.0, 35.0]]]], np.float32)
    got = draw_poses_np(fr, kp, None, segments=[[0, 0]], colors=[[9, 9, 9]], dot_color=(1, 1, 1), thickness=1, dot_radius=r)[0, :, :, 0]
    disc = got != 0
    assert np.array_equal(disc, disc[::-1]) and np.array_equal(disc, disc[:, ::-1]) and np.array_equal(disc, disc.T)
    for y in range(71):
        for x in range(71):
            assert disc[y, x] == ((x - 35) ** 2 + (y - 35) ** 2 <= r * r)
    assert disc.sum() == sum(1 for y in range(-r, r + 1) for x in range(-r, r + 1) if x * x + y * y <= r * r)


# ---- order and visibility ----
def test_paint_order_is_plot_on_frames_loop():
    fr = np.zeros((1, 40, 40, 3), np.uint8)
    kp = np.array([[[[10.0, 20.0], [30.0, 20.0]], [[20.0, 5.0], [20.0, 35.0]]]], np.float32)           # person 0 horizontal, person 1 vertical, crossing at (20, 20)
    seg, col = [[0, 1]], [[0, 0, 200]]
    got = draw_poses_np(fr, kp, None, segments=seg, colors=col, dot_color=(255, 255, 255), thickness=3, dot_radius=4,
                        fills=[[0, 0, 40, 40, 50, 50, 50], [15, 15, 25, 25, 60, 60, 60]])[0]
    assert tuple(got[0, 0]) == (50, 50, 50) and tuple(got[16, 16]) == (60, 60, 60), "fills first, in their own order"
    assert tuple(got[20, 20]) == (0, 0, 200), "person 1's line over person 0's line"
    assert tuple(got[20, 10]) == (255, 255, 255), "a person's dots over its own line"
    kp2 = kp.copy()
    kp2[0, 1] = [[10.0, 5.0], [10.0, 35.0]]                                                          # person 1's line now crosses person 0's first dot
    got = draw_poses_np(fr, kp2, None, segments=seg, colors=col, dot_color=(255, 255, 255), thickness=3, dot_radius=4)[0]
    assert tuple(got[20, 10]) == (0, 0, 200), "a later person's line over an earlier person's dot"
    assert tuple(got[20, 13]) == (255, 255, 255), "the rest of the dot stays"
    got = draw_poses_np(fr, kp2[:, ::-1], None, segments=seg, colors=col, dot_color=(255, 255, 255), thickness=3, dot_radius=4)[0]
    assert tuple(got[20, 10]) == (255, 255, 255), "and the other way round with the persons swapped"


def test_visibility():
    assert int(-0.5) == 0 and joint_pixel(-0.5, -0.99) == (0, 0) and joint_pixel(3.99, -1.0) == (3, -1)
    for bad in ((math.nan, 1.0), (1.0, math.inf), (-math.inf, 1.0), (-32769.0, 0.0), (0.0, 65536.0), (1e30, 0.0)):
        assert joint_pixel(*bad) is None, bad
    assert joint_pixel(-32768.9, 65535.9) == (-32768, 65535)
    assert joint_pixel(1.0, 1.0, 0.3, 0.3) is None and joint_pixel(1.0, 1.0, math.nan, 0.3) is None and joint_pixel(1.0, 1.0, 0.31, 0.3) == (1, 1)
    assert joint_pixel(1.0, 1.0, 0.0, math.nan) == (1, 1) and joint_pixel(1.0, 1.0, math.nan, None) == (1, 1)
    fr = np.zeros((1, 20, 20, 3), np.uint8)
    kw = dict(segments=[[0, 1]], colors=[[5, 5, 5]], dot_color=(9, 9, 9), thickness=1, dot_radius=0)
    kp = np.array([[[[-0.5, -0.5, 1.0], [6.0, 0.0, 0.2]]]], np.float32)
    got = draw_poses_np(fr, kp, None, min_score=0.25, **kw)[0]
    assert tuple(got[0, 0]) == (9, 9, 9) and not got[0, 1:].any(), "the low-score joint takes its dot and the line with it"
    got = draw_poses_np(fr, kp, None, min_score=None, **kw)[0]
    assert tuple(got[0, 3]) == (5, 5, 5) and tuple(got[0, 6]) == (9, 9, 9)
    assert not draw_poses_np(fr, kp, np.zeros((1, 1), np.uint8), **kw).any(), "valid == 0"
    kp[0, 0, 1, 0] = np.nan
    got = draw_poses_np(fr, kp, None, **kw)[0]
    assert tuple(got[0, 0]) == (9, 9, 9) and got.sum() == 27, "a NaN joint: its dot and its line are gone, the other dot stays"


# ---- the tables ----
def header_tables():
    hdr = open(os.path.join(ROOT, "include", "kasf.h")).read()
    found = {}
    for m in re.finditer(r"#define\s+KASF_RGB2YUV_COEF_(BT601|BT709)_(LIMITED|FULL)\s*\{([^}]*)\}", hdr):
        found[(m[1].lower(), m[2] == "FULL")] = tuple(int(v) for v in m[3].split(","))
    return found


def test_header_literals_are_the_rounded_formulas():
    found = header_tables()
    assert found == TABLES, "include/kasf.h and the restatement hold the same four tables"
    for key, t in TABLES.items():
        assert t == tuple(int(np.rint(c * 2.0 ** 20)) for c in exact_coefficients(*key)), key
        # rule 5's int32 bound
        assert 255 * (t[0] + t[1] + t[2]) + (16 << 20) + (1 << 19) < 2.9e8
        for row in ((t[3], t[4], t[5]), (t[5], t[6], t[7])):
            hi = 1020 * sum(c for c in row if c > 0) + (128 << 22) + (1 << 21)
            lo = 1020 * sum(c for c in row if c < 0) + (128 << 22) + (1 << 21)
            assert -2 ** 31 < lo <= hi < 2 ** 31
    from kasportsformer_amd import draw
    assert tuple(map(tuple, np.asarray(draw.H36M_SEGMENTS))) == H36M_SEGMENTS


EPS = 1e-9        # the fp64 evaluation of the exact conversion itself


@pytest.mark.parametrize("matrix,full_range", sorted(TABLES))
def test_luma_and_chroma_are_within_the_computed_bound_of_the_exact_conversion(matrix, full_range):
    """Luma over all 2^24 (B, G, R); chroma over all 2^24 uniform quads (sums = 4 x the colour) and 10^6 random quads, against the exact fp64 conversion of the
    pixel / of the quad's mean, clamped.  Bounds (Y, U, V), computed from the tables, and the measured worst distances:
      bt601 limited  0.5001 0.5000 0.5000   measured 0.50006 0.50000 0.50000 (all colours), 0.50000 0.50000 (random quads U, V)
      bt601 full     0.5002 0.5002 0.5001   measured 0.5 0.5 0.5, 0.5 0.5
      bt709 limited  0.5002 0.5002 0.5001   measured 0.50017 0.50008 0.50002, 0.50002 0.50000
      bt709 full     0.5002 0.5002 0.5001   measured 0.5 0.5 0.5, 0.5 0.5"""
    by, bu, bv = nv12_bound(matrix, full_range)
    assert max(by, bu, bv) < 0.5004
    k = exact_coefficients(matrix, full_range)
    yoff = 0.0 if full_range else 16.0
    G, R = np.arange(256)[:, None], np.arange(256)[None, :]
    worst = np.zeros(3)
    for B in range(256):
        px = np.empty((1, 256, 256, 3), np.uint8)
        px[0, :, :, 0], px[0, :, :, 1], px[0, :, :, 2] = B, G, R
        y, _ = bgr_to_nv12_np(px, matrix, full_range)
        quad = np.repeat(np.repeat(px.reshape(256 * 256, 1, 1, 3), 2, axis=1), 2, axis=2)                # every colour as a uniform 2 x 2 frame
        _, uv = bgr_to_nv12_np(quad, matrix, full_range)
        r, g, b = R.astype(np.float64), G.astype(np.float64), float(B)
        wy = np.clip(yoff + k[0] * r + k[1] * g + k[2] * b, 0, 255)
        wu = np.clip(128.0 + k[3] * r + k[4] * g + k[5] * b, 0, 255)
        wv = np.clip(128.0 + k[5] * r + k[6] * g + k[7] * b, 0, 255)
        worst = np.maximum(worst, [np.abs(y[0] - wy).max(), np.abs(uv[:, 0, 0, 0].reshape(256, 256) - wu).max(), np.abs(uv[:, 0, 0, 1].reshape(256, 256) - wv).max()])
    g = np.random.default_rng(11)
    quads = g.integers(0, 256, size=(10 ** 6, 2, 2, 3), dtype=np.uint8)
    _, uv = bgr_to_nv12_np(quads, matrix, full_range)
    mean = quads.astype(np.float64).mean(axis=(1, 2))                                                   # exact: sums of four bytes over 4
    wu = np.clip(128.0 + k[3] * mean[:, 2] + k[4] * mean[:, 1] + k[5] * mean[:, 0], 0, 255)
    wv = np.clip(128.0 + k[5] * mean[:, 2] + k[6] * mean[:, 1] + k[7] * mean[:, 0], 0, 255)
    rand = [np.abs(uv[:, 0, 0, 0] - wu).max(), np.abs(uv[:, 0, 0, 1] - wv).max()]
    print(f"{matrix} full_range={full_range}: bounds {by:.4f} {bu:.4f} {bv:.4f}, measured {worst}, random quads {rand}")
    assert worst[0] <= by + EPS and worst[1] <= bu + EPS and worst[2] <= bv + EPS
    assert rand[0] <= bu + EPS and rand[1] <= bv + EPS


def test_a_wrong_matrix_violates_the_bound_and_rgb_swaps_the_ends():
    fr = noise_frames(1, 9, 11, 3)
    y, uv = bgr_to_nv12_np(fr)
    y2, uv2 = bgr_to_nv12_np(fr[..., ::-1], rgb=True)
    assert np.array_equal(y, y2) and np.array_equal(uv, uv2)
    assert uv.shape == (1, 5, 6, 2) and y.shape == (1, 9, 11)
    y709, _ = bgr_to_nv12_np(fr, matrix="bt709")
    assert np.abs(y.astype(int) - y709.astype(int)).max() > 2
    # an odd edge replicates: the last chroma column of the 11-wide frame is that of the frame with its last column doubled
    wide = np.concatenate([fr, fr[:, :, -1:]], axis=2)
    tall = np.concatenate([wide, wide[:, -1:]], axis=1)
    assert np.array_equal(bgr_to_nv12_np(tall)[1], uv)


# ---- the panel ----
def test_panel_is_the_orthographic_view():
    from kasportsformer_amd.draw import panel_view
    g = np.random.default_rng(5)
    world = g.normal(0.0, 0.4, size=(6, 17, 3)).astype(np.float32)
    for rect, elev, azim, radius in (((1280, 0, 1920, 640), 5.0, 5.0, 0.72), ((0, 0, 100, 300), 15.0, 70.0, 1.0), ((10.5, 20.5, 500.5, 400.0), -30.0, 200.0, 0.5)):
        view = panel_view(rect, elev, azim, radius)
        assert view.dtype == np.float32 and view.shape == (8,)
        got = pose_panel_np(world, view)
        el, az = math.radians(elev), math.radians(azim)
        right = np.array([-math.sin(az), math.cos(az), 0.0])
        up = np.array([-math.sin(el) * math.cos(az), -math.sin(el) * math.sin(az), math.cos(el)])
        assert abs(right @ up) < 1e-15 and abs(up @ up - 1) < 1e-15
        scale = min(rect[2] - rect[0], rect[3] - rect[1]) / 2 / radius
        d = world.astype(np.float64) - world[:, :1].astype(np.float64)
        want = np.stack(((rect[0] + rect[2]) / 2 + scale * (d @ right), (rect[1] + rect[3]) / 2 - scale * (d @ up)), axis=-1)
        size = max(abs(v) for v in rect) + scale * np.abs(d).max() * 3
        assert np.abs(got - want).max() <= 8 * np.finfo(np.float32).eps * size, (np.abs(got - want).max(), size)
        assert np.array_equal(got[:, 0], np.broadcast_to(view[6:8], (6, 2))), "the root joint sits at the panel's centre"
    with pytest.raises(ValueError):
        panel_view((0, 0, 0, 10))
    with pytest.raises(ValueError):
        panel_view((0, 0, 10, 10), radius=0.0)
    with pytest.raises(TypeError):
        panel_view(5)


# ---- refusals ----
def _call_draw(lib, buf, **over):
    p = buf.ctypes.data_as(C.c_void_p)
    a = dict(frames=p, n_frames=2, Hf=4, Wf=6, row_stride=18, frame_stride=72, keypoints=p, P=2, J=17, C=3, kp_f=102, kp_p=51, kp_j=3, kp_c=1, valid=p, v_f=2, v_p=1,
             segments=p, colors=p, S=16, dot=p, t=2, r=2, min_score=0.5, fills=p, R=1, out=p, o_rs=18, o_fs=72, oy=p, ouv=p, y_rs=6, uv_rs=6, y_fs=24, uv_fs=12,
             matrix=0, full_range=0, rgb=0)
    a.update(over)
    return lib.kasf_draw_poses(*a.values(), None)


def test_c_entry_points_refuse_without_a_device():
    """Every error-2 condition of include/kasf.h, through the C-ABI; the pointers are host memory, which must come back unchanged (nothing is touched)."""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    bad = [dict(n_frames=-1), dict(Hf=0), dict(Hf=32768), dict(Wf=0), dict(Wf=32768), dict(row_stride=17), dict(o_rs=17), dict(y_rs=5), dict(uv_rs=5),
           dict(Wf=5, row_stride=15, o_rs=15, uv_rs=5),                                   # 2 * ((5 + 1) / 2) = 6 chroma bytes
           dict(frame_stride=-1), dict(o_fs=-1), dict(y_fs=-1), dict(uv_fs=-1), dict(frame_stride=71), dict(o_fs=71), dict(y_fs=23), dict(uv_fs=11),
           dict(out=None, oy=None, ouv=None), dict(oy=None), dict(ouv=None), dict(P=-1), dict(P=(1 << 20) + 1), dict(S=-1), dict(S=33), dict(J=0), dict(J=33),
           dict(C=1), dict(C=4), dict(keypoints=None), dict(segments=None), dict(colors=None), dict(dot=None), dict(t=0), dict(t=65), dict(r=-1), dict(r=33),
           dict(R=-1), dict(R=9), dict(fills=None), dict(matrix=2), dict(matrix=-1), dict(frames=None)]
    for over in bad:
        assert _call_draw(lib, buf, **over) == 2, over
        assert lib.kasf_last_error()
    assert _call_draw(lib, buf, n_frames=0) == 0, "no frames: nothing to do"
    assert _call_draw(lib, buf, n_frames=0, frames=None) == 0
    assert _call_draw(lib, buf, row_stride=2 ** 62, frame_stride=2 ** 62) == 2, "no overflow in the check itself"
    p = buf.ctypes.data_as(C.c_void_p)

    def nv12(**over):
        a = dict(frames=p, n_frames=2, Hf=4, Wf=6, row_stride=18, frame_stride=72, oy=p, ouv=p, y_rs=6, uv_rs=6, y_fs=24, uv_fs=12, matrix=0, full_range=0, rgb=0)
        a.update(over)
        return lib.kasf_bgr_to_nv12(*a.values(), None)
    for over in (dict(n_frames=-1), dict(Hf=0), dict(Wf=32768), dict(row_stride=17), dict(y_rs=5), dict(uv_rs=5), dict(frame_stride=71), dict(y_fs=23), dict(uv_fs=11),
                 dict(oy=None), dict(ouv=None), dict(matrix=3), dict(frames=None)):
        assert nv12(**over) == 2, over
    assert nv12(n_frames=0) == 0
    view = (C.c_float * 8)(1, 0, 0, 0, 1, 0, 5, 5)
    fp = buf.ctypes.data_as(C.c_void_p)
    assert lib.kasf_pose_panel(fp, -1, view, fp, None) == 2 and lib.kasf_pose_panel(fp, (1 << 40) + 1, view, fp, None) == 2
    assert lib.kasf_pose_panel(fp, 1, None, fp, None) == 2 and lib.kasf_pose_panel(None, 1, view, fp, None) == 2 and lib.kasf_pose_panel(fp, 1, view, None, None) == 2
    for i in range(8):
        v = (C.c_float * 8)(1, 0, 0, 0, 1, 0, 5, 5)
        v[i] = math.nan if i % 2 else math.inf
        assert lib.kasf_pose_panel(fp, 1, v, fp, None) == 2, i
    assert lib.kasf_pose_panel(None, 0, view, None, None) == 0
    assert not buf.any()
    assert lib.kasf_version() == 12


def test_python_checks_refuse_without_a_device():
    import kasportsformer_amd as K
    fr = np.zeros((8, 8, 3), np.uint8)
    kp = np.zeros((2, 17, 3), np.float32)
    for args, kw, exc in (
            ((fr.astype(np.float32), kp), {}, TypeError), ((fr[..., :2], kp), {}, ValueError), ((fr, kp[None]), {}, ValueError), ((fr, kp.astype(np.int32)), {}, TypeError),
            ((fr, np.zeros((2, 33, 2), np.float32)), {}, ValueError), ((fr, np.zeros((2, 17, 4), np.float32)), {}, ValueError), ((fr, "kp"), {}, TypeError),
            ((fr, kp, np.zeros(3, np.uint8)), {}, ValueError), ((fr, kp, np.zeros(2, np.float32)), {}, TypeError),
            ((fr, kp), dict(segments=[[0, 17]]), ValueError), ((fr, kp), dict(segments=[[0, 1]], colors=[[1, 2, 3], [4, 5, 6]]), ValueError),
            ((fr, kp), dict(segments=[[0.5, 1]]), TypeError), ((fr, kp), dict(segments=np.zeros((33, 2), np.int32), colors=np.zeros((33, 3), np.uint8)), ValueError),
            ((fr, kp), dict(colors=np.full((16, 3), 256)), ValueError), ((fr, kp), dict(dot_color=(1, 2)), TypeError), ((fr, kp), dict(dot_color=(1, 2, 256)), ValueError),
            ((fr, kp), dict(thickness=0), ValueError), ((fr, kp), dict(thickness=65), ValueError), ((fr, kp), dict(thickness=2.0), TypeError),
            ((fr, kp), dict(dot_radius=-1), ValueError), ((fr, kp), dict(dot_radius=33), ValueError), ((fr, kp), dict(min_score="x"), TypeError),
            ((fr, kp), dict(fills=np.zeros((9, 7), np.int32)), ValueError), ((fr, kp), dict(fills=[[0, 0, 1, 1, 0, 0]]), ValueError),
            ((fr, kp), dict(out=np.zeros_like(fr)), TypeError), ((fr, kp), dict(out=torch.zeros(8, 8, 3, dtype=torch.uint8)), RuntimeError),
            ((fr, kp), dict(out=torch.zeros(8, 9, 3, dtype=torch.uint8)), ValueError), ((fr, kp), dict(out=False), ValueError),
            ((fr, kp), dict(surface=(torch.zeros(8, 8, dtype=torch.uint8),)), ValueError), ((fr, kp), dict(surface="yes"), TypeError),
            ((fr, kp), dict(surface=(torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(4, 4, 2, dtype=torch.uint8))), RuntimeError),
            ((fr, kp), dict(matrix="bt2020"), ValueError)):
        with pytest.raises(exc):
            K.draw_poses(*args, **kw)
    with pytest.raises(ValueError):
        K.bgr_to_nv12(fr, matrix="x")
    with pytest.raises(TypeError):
        K.bgr_to_nv12(fr.astype(np.int16))
    with pytest.raises(ValueError):
        K.poses_to_panel(np.zeros((2, 16, 3), np.float32), (0, 0, 10, 10))
    with pytest.raises(TypeError):
        K.poses_to_panel(np.zeros((2, 17, 3), np.int32), (0, 0, 10, 10))
    if not torch.cuda.is_available():
        for call in (lambda: K.draw_poses(fr, kp), lambda: K.bgr_to_nv12(fr), lambda: K.poses_to_panel(np.zeros((1, 17, 3), np.float32), (0, 0, 10, 10))):
            with pytest.raises(RuntimeError, match="no GPU"):
                call()
    pal = K.draw.hue_wheel(16)
    assert pal.shape == (16, 3) and pal.dtype == np.uint8 and len({tuple(c) for c in pal}) == 16 and tuple(pal[0]) == (0, 0, 255)
