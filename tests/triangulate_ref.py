"""Shared by tests/test_triangulate_cpu.py, tests/test_triangulate_host_cpu.py, tests/test_gpu_triangulate.py and tools/triangulate_bench.py (not a test): the
rule of include/kasf.h's kasf_keypoints_triangulate / kasf_keypoints_undistort in numpy -- fp64, one numpy operation per rounded operation of the rule, views
in ascending order, fp32 rounding at the stores only -- and the generators of its tests: cameras on a ring, a forward projection with the Brown-Conrady
distortion, and a ``bundle`` of frames that contains every state.

``triangulate_point`` is the rule as a scalar loop over one point in the header's order, in Python floats (fp64).  ``triangulate_np`` is the same arithmetic
over all points at once -- a view that is not usable is masked out of a sum where the scalar loop skips it, and the state is read off the header's list at the
end -- because a Python loop over the 65,000 view-points of the larger device cases takes minutes; tests/test_triangulate_cpu.py holds the two to one another
bit for bit.  The text differs from the kernel's on purpose."""
import math

import numpy as np

LIMIT = np.float32(1e12)
PIVOT = 1e-9
HUGE = np.finfo(np.float64).max
FMAX = np.finfo(np.float32).max
OK, TOO_FEW, DEGENERATE, BEHIND = 0, 1, 2, 3
NAN32 = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
DEFAULTS = dict(min_score=0.3, weighted=True, iterations=4, delta=3.0, min_views=2, undistort_iterations=5)
LENS = np.array([-0.12, 0.05, 0.001, -0.0005, 0.01], np.float32)       # k1, k2, p1, p2, k3 of a wide action-camera lens


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def camera_row(intrinsics, distortion, R, t):
    """fx, fy, cx, cy | k1, k2, p1, p2, k3 | R row-major | t -> float32 [..., 21]."""
    R = np.asarray(R, np.float32)
    return np.concatenate([np.asarray(intrinsics, np.float32), np.asarray(distortion, np.float32), R.reshape(R.shape[:-2] + (9,)), np.asarray(t, np.float32)], -1)


def _undistort64(cam, u, v, rounds):
    """cam [..., >= 9] fp64, u, v fp64 -> the undistorted normalised x, y (fp64), the header's lines."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (cam[..., i] for i in range(9))
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd, yd
    for _ in range(rounds):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return x, y


def undistort_np(K, camera, ppf=1, iterations=5):
    """kasf_keypoints_undistort over K [M,3] fp32; camera [9] or [M // ppf, 9] fp32 -> [M,3] fp32."""
    K = np.ascontiguousarray(K, np.float32).reshape(-1, 3)
    M = len(K)
    cam32 = np.asarray(camera, np.float32).reshape(-1, 9)
    cam32 = np.repeat(cam32, ppf, 0) if len(cam32) > 1 else np.broadcast_to(cam32, (M, 9))
    with np.errstate(all="ignore"):
        ok = (np.abs(K[:, :2]) <= LIMIT).all(1) & (np.abs(cam32) <= FMAX).all(1)
        cam = cam32.astype(np.float64)
        x, y = _undistort64(cam, K[:, 0].astype(np.float64), K[:, 1].astype(np.float64), iterations)
        out = K.copy()
        out[:, 0] = np.where(ok, (cam[:, 0] * x + cam[:, 2]).astype(np.float32), K[:, 0])
        out[:, 1] = np.where(ok, (cam[:, 1] * y + cam[:, 3]).astype(np.float32), K[:, 1])
    return out


def _cams(cameras, C, M, ppf):
    """cameras [C,21] or [C, M // ppf, 21] fp32 -> [C, M, 21] fp32."""
    cam = np.asarray(cameras, np.float32)
    return np.broadcast_to(cam[:, None, :], (C, M, 21)) if cam.ndim == 2 else np.repeat(cam, ppf, 1)


def triangulate_np(K, cameras, ppf=1, min_score=0.3, weighted=True, iterations=4, delta=3.0, min_views=2, undistort_iterations=5):
    """The rule over K [C,M,3] fp32 and cameras [C,21] or [C, M // ppf, 21] fp32 ->
    dict(points [M,3], residual [M], view_residual [C,M], all fp32, used [M] and state [M] uint8)."""
    K = np.ascontiguousarray(K, np.float32)
    C, M = K.shape[:2]
    cam32 = _cams(cameras, C, M, ppf)
    with np.errstate(all="ignore"):
        use = (np.abs(K[..., :2]) <= LIMIT).all(-1) & (K[..., 2] >= np.float32(min_score)) & (np.abs(cam32) <= FMAX).all(-1)        # step 1, [C,M]
        cam = cam32.astype(np.float64)
        x, y = _undistort64(cam, K[..., 0].astype(np.float64), K[..., 1].astype(np.float64), undistort_iterations)
        fx, fy = cam[..., 0], cam[..., 1]
        R, t = cam[..., 9:18], cam[..., 18:21]
        w0 = K[..., 2].astype(np.float64) if weighted else np.ones((C, M))
        d2 = np.float64(np.float32(delta)) * np.float64(np.float32(delta))
        X = np.zeros((3, M))
        flat, behind = np.zeros(M, bool), np.zeros(M, bool)

        def rho_at(c):                                                  # step 3's rho of view c at X, its depth, and whether it is in front
            Xc = R[c, :, 0] * X[0] + R[c, :, 1] * X[1] + R[c, :, 2] * X[2] + t[c, :, 0]
            Yc = R[c, :, 3] * X[0] + R[c, :, 4] * X[1] + R[c, :, 5] * X[2] + t[c, :, 1]
            Zc = R[c, :, 6] * X[0] + R[c, :, 7] * X[1] + R[c, :, 8] * X[2] + t[c, :, 2]
            du, dv = fx[c] * (Xc / Zc - x[c]), fy[c] * (Yc / Zc - y[c])
            return du * du + dv * dv, Zc, Zc > 0.0

        for it in range(iterations + 1):                                # steps 2 and 3
            S = [np.zeros(M) for _ in range(9)]                         # A00 A01 A02 A11 A12 A22 b0 b1 b2
            for c in range(C):
                u = use[c]
                wu, wv = w0[c] * (fx[c] * fx[c]), w0[c] * (fy[c] * fy[c])
                if it > 0:
                    rho, Zc, front = rho_at(c)
                    behind |= u & ~front
                    g, z2 = w0[c] / (1.0 + rho / d2), Zc * Zc
                    wu, wv = g * (fx[c] * fx[c]) / z2, g * (fy[c] * fy[c]) / z2
                rows = ((wu, x[c] * R[c, :, 6] - R[c, :, 0], x[c] * R[c, :, 7] - R[c, :, 1], x[c] * R[c, :, 8] - R[c, :, 2], t[c, :, 0] - x[c] * t[c, :, 2]),
                        (wv, y[c] * R[c, :, 6] - R[c, :, 3], y[c] * R[c, :, 7] - R[c, :, 4], y[c] * R[c, :, 8] - R[c, :, 5], t[c, :, 1] - y[c] * t[c, :, 2]))
                for w, a0, a1, a2, r in rows:
                    terms = (a0 * a0, a0 * a1, a0 * a2, a1 * a1, a1 * a2, a2 * a2, a0 * r, a1 * r, a2 * r)
                    S = [np.where(u, s + w * term, s) for s, term in zip(S, terms)]
            A00, A01, A02, A11, A12, A22, b0, b1, b2 = S
            floor = PIVOT * (A00 + A11 + A22)
            d0 = A00
            l10, l20 = A01 / d0, A02 / d0
            d1 = A11 - l10 * A01
            m12 = A12 - l10 * A02
            l21 = m12 / d1
            dd2 = A22 - l20 * A02 - l21 * m12
            flat |= ~(d0 > floor) | ~(d1 > floor) | ~(dd2 > floor)
            c1 = b1 - l10 * b0
            c2 = b2 - l20 * b0 - l21 * c1
            X2 = c2 / dd2
            X1 = c1 / d1 - l21 * X2
            X0 = b0 / d0 - l10 * X1 - l20 * X2
            X = np.stack([X0, X1, X2])
            flat |= ~(np.abs(X) <= HUGE).all(0)
        num, den = np.zeros(M), np.zeros(M)                              # step 4
        view = np.zeros((C, M))
        for c in range(C):
            rho, _, front = rho_at(c)
            behind |= use[c] & ~front
            num = np.where(use[c], num + w0[c] * rho, num)
            den = np.where(use[c], den + w0[c], den)
            view[c] = np.sqrt(rho)
        used = use.sum(0)
        state = np.where(used < min_views, TOO_FEW, np.where(flat, DEGENERATE, np.where(behind, BEHIND, OK))).astype(np.uint8)
        ok = state == OK
        points = np.where(ok[:, None], X.T.astype(np.float32), NAN32)
        residual = np.where(ok, np.sqrt(num / den).astype(np.float32), NAN32)
        view_residual = np.where(ok[None, :] & use, view.astype(np.float32), NAN32)
    return dict(points=np.ascontiguousarray(points), residual=residual, used=used.astype(np.uint8), state=state, view_residual=view_residual)


def triangulate_point(k, cams, min_score=0.3, weighted=True, iterations=4, delta=3.0, min_views=2, undistort_iterations=5):
    """One point: k [C,3] fp32, cams [C,21] fp32 -> (X fp32 [3], residual fp32, used, state, view_residual fp32 [C]): the header's steps as a scalar loop."""
    C = len(k)
    inf, nan = math.inf, math.nan

    def div(a, b):                                                       # IEEE division where Python raises
        if b == 0.0:
            return nan if (a == 0.0 or a != a) else math.copysign(inf, a) * math.copysign(1.0, b)
        return a / b

    views = []
    for c in range(C):
        usable = bool(abs(k[c, 0]) <= LIMIT and abs(k[c, 1]) <= LIMIT and k[c, 2] >= np.float32(min_score) and (np.abs(cams[c]) <= FMAX).all())
        if not usable:
            views.append(None)
            continue
        cam = [float(v) for v in cams[c]]
        fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam[:9]
        xd, yd = div(float(k[c, 0]) - cx, fx), div(float(k[c, 1]) - cy, fy)
        x, y = xd, yd
        for _ in range(undistort_iterations):
            r2 = x * x + y * y
            rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = div(xd - dx, rad), div(yd - dy, rad)
        views.append((x, y, float(k[c, 2]) if weighted else 1.0, fx, fy, cam[9:18], cam[18:21]))
    used = sum(v is not None for v in views)
    d2 = float(np.float32(delta)) * float(np.float32(delta))
    X0 = X1 = X2 = 0.0
    flat = behind = False
    num = den = 0.0
    vr = [nan] * C
    for it in range(iterations + 2):
        last = it == iterations + 1
        S = [0.0] * 9
        for c, view in enumerate(views):
            if view is None:
                continue
            x, y, w0, fx, fy, R, t = view
            wu, wv = w0 * (fx * fx), w0 * (fy * fy)
            if it > 0:
                Xc = R[0] * X0 + R[1] * X1 + R[2] * X2 + t[0]
                Yc = R[3] * X0 + R[4] * X1 + R[5] * X2 + t[1]
                Zc = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2]
                if not Zc > 0.0:
                    behind = True
                du, dv = fx * (div(Xc, Zc) - x), fy * (div(Yc, Zc) - y)
                rho = du * du + dv * dv
                if last:
                    num, den = num + w0 * rho, den + w0
                    vr[c] = math.sqrt(rho) if rho >= 0.0 else nan
                    continue
                g, z2 = div(w0, 1.0 + div(rho, d2)), Zc * Zc
                wu, wv = div(g * (fx * fx), z2), div(g * (fy * fy), z2)
            for w, a0, a1, a2, r in ((wu, x * R[6] - R[0], x * R[7] - R[1], x * R[8] - R[2], t[0] - x * t[2]),
                                     (wv, y * R[6] - R[3], y * R[7] - R[4], y * R[8] - R[5], t[1] - y * t[2])):
                for i, term in enumerate((a0 * a0, a0 * a1, a0 * a2, a1 * a1, a1 * a2, a2 * a2, a0 * r, a1 * r, a2 * r)):
                    S[i] = S[i] + w * term
        if last:
            break
        A00, A01, A02, A11, A12, A22, b0, b1, b2 = S
        floor = PIVOT * (A00 + A11 + A22)
        d0 = A00
        l10, l20 = div(A01, d0), div(A02, d0)
        d1 = A11 - l10 * A01
        m12 = A12 - l10 * A02
        l21 = div(m12, d1)
        dd2 = A22 - l20 * A02 - l21 * m12
        if not d0 > floor or not d1 > floor or not dd2 > floor:
            flat = True
        c1 = b1 - l10 * b0
        c2 = b2 - l20 * b0 - l21 * c1
        X2 = div(c2, dd2)
        X1 = div(c1, d1) - l21 * X2
        X0 = div(b0, d0) - l10 * X1 - l20 * X2
        if not (abs(X0) <= HUGE and abs(X1) <= HUGE and abs(X2) <= HUGE):
            flat = True
    state = TOO_FEW if used < min_views else DEGENERATE if flat else BEHIND if behind else OK
    if state != OK:
        return np.full(3, NAN32), NAN32, used, state, np.full(C, NAN32)
    with np.errstate(all="ignore"):
        q = div(num, den)
        return (np.array([X0, X1, X2]).astype(np.float32), np.float32(math.sqrt(q) if q >= 0.0 else nan), used, state,
                np.array([NAN32 if v is None else np.float32(r) for v, r in zip(views, vr)], np.float32))


# ---- generators ----

def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """A camera at `eye` that looks at `target` (x right, y down, z forward) -> (R [3,3], t [3]) fp64 with X_cam = R X_world + t."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ eye


def ring(views, rng=None, radius=12.0, height=4.0, f=1500.0, size=(1920.0, 1080.0), distortion=None):
    """`views` cameras on a ring of `radius` metres at `height`, looking at a point a metre above the centre -> float32 [views, 21]."""
    rows = []
    for c in range(views):
        a = 2.0 * np.pi * c / views + (0.0 if rng is None else rng.uniform(-0.1, 0.1))
        r = radius * (1.0 if rng is None else rng.uniform(0.9, 1.1))
        R, t = look_at((r * np.cos(a), r * np.sin(a), height), (0.0, 0.0, 1.0))
        fc = f * (1.0 if rng is None else rng.uniform(0.9, 1.1))
        rows.append(camera_row([fc, fc, size[0] / 2, size[1] / 2], np.zeros(5) if distortion is None else distortion, R, t))
    return np.stack(rows)


def project(X, cams):
    """World points X [M,3] fp64 through cams [C,21] or [C,M,21] with the forward Brown-Conrady distortion -> pixels [C,M,2] in fp64."""
    cam = np.asarray(cams, np.float64)
    cam = cam[:, None, :] if cam.ndim == 2 else cam
    R, t = cam[..., 9:18], cam[..., 18:21]
    Xc = R[..., 0] * X[:, 0] + R[..., 1] * X[:, 1] + R[..., 2] * X[:, 2] + t[..., 0]
    Yc = R[..., 3] * X[:, 0] + R[..., 4] * X[:, 1] + R[..., 5] * X[:, 2] + t[..., 1]
    Zc = R[..., 6] * X[:, 0] + R[..., 7] * X[:, 1] + R[..., 8] * X[:, 2] + t[..., 2]
    x, y = Xc / Zc, Yc / Zc
    k1, k2, p1, p2, k3 = (cam[..., 4 + i] for i in range(5))
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return np.stack([cam[..., 0] * xd + cam[..., 2], cam[..., 1] * yd + cam[..., 3]], -1)


def players(rng, frames, joints=17, spread=4.0):
    """`frames` players spread over a few metres, each a cloud of `joints` joints within a metre -> [frames * joints, 3] fp64 world points."""
    centre = np.concatenate([rng.uniform(-spread, spread, (frames, 2)), rng.uniform(0.8, 1.2, (frames, 1))], 1)
    return (centre[:, None, :] + rng.uniform(-0.8, 0.8, (frames, joints, 3))).reshape(-1, 3)


def bundle(frames, views, seed=0, per_frame=False, distortion=None, joints=17):
    """A synthetic rig and one player's keypoints in it: (keypoints [views, frames * joints, 3] fp32, cameras [views,21] or [views,frames,21] fp32, X_true
    [frames * joints, 3] fp64).  Cameras on a ring about 12 m from players spread over a few metres, f about 1500 px, a pixel of noise, scores in [0.5, 1], low
    scores and NaN keypoints now and then.  With views >= 3 the last camera is a second feed of camera 0 (the same row).  Planted, by frame index f:
    f % 5 == 1: joint j keeps only its first (j + f // 5) % (views + 1) views, so `used` takes every value from 0 to `views`; f % 5 == 3 (of frames with fewer than 7 joints: f % 15 == 3, and == 4 below), joints 0 - 3, with
    views >= 3: only camera 0 and its second feed see the joint, at the same pixel -- rays that do not spread, state 2; f % 5 == 4, joints 5 and 6 (joint 0 of a one-joint frame): a point
    8 m behind camera 0, seen by it and by the camera most nearly opposite only (state 3); f % 7 == 2: view 1's keypoint of joint 9 is displaced by 120 px; per_frame, f % 6 == 5: view 1's camera has a NaN."""
    rng = np.random.default_rng(2000 + seed)
    lens = np.zeros(5, np.float32) if distortion is None else np.asarray(distortion, np.float32)
    cams = ring(views, rng, distortion=lens)
    if views >= 3:
        cams[-1] = cams[0]
    X = players(rng, frames, joints)
    M = frames * joints
    f, j = np.repeat(np.arange(frames), joints), np.tile(np.arange(joints), frames)
    rare = 5 if joints > 6 else 15                                       # a one-joint frame is all planted or not at all: plant fewer of them
    far = (f % rare == 4) & (((j == 5) | (j == 6)) if joints > 6 else (j == 0))
    partner = views // 2                                                 # the camera most nearly opposite camera 0
    if far.any():
        eye = [-(cams[c, 9:18].reshape(3, 3).astype(np.float64).T @ cams[c, 18:21].astype(np.float64)) for c in (0, partner)]
        back = (eye[0] - eye[1]) / np.linalg.norm(eye[0] - eye[1])
        X[far] = eye[0] + 8.0 * back + rng.uniform(-0.5, 0.5, (int(far.sum()), 3))
    if per_frame:
        cams = np.repeat(cams[:, None, :], frames, 1)
        cams[:, :, :2] *= rng.uniform(0.95, 1.05, (1, frames, 1)).astype(np.float32)         # a zoom that every camera follows, frame by frame
        cams[:, :, 18:21] += rng.normal(0.0, 0.01, (views, frames, 3)).astype(np.float32)
        if views >= 3:
            cams[-1] = cams[0]
        cams[1, np.arange(frames) % 6 == 5, 12] = np.nan
    uv = project(X, np.repeat(cams, joints, 1) if per_frame else cams)
    K = np.concatenate([uv + rng.normal(0.0, 1.0, uv.shape), rng.uniform(0.5, 1.0, (views, M, 1))], -1).astype(np.float32)
    K[..., 2] = np.where(rng.random((views, M)) < 0.05, rng.uniform(0.0, 0.29, (views, M)), K[..., 2]).astype(np.float32)
    K[0, (f % 10 == 0) & (j == 2), 0] = np.nan
    K[1, (f % 7 == 2) & (j == 9), :2] += np.float32(120.0)
    keep = (j + f // 5) % (views + 1)
    for c in range(views):
        K[c, (f % 5 == 1) & (c >= keep), 2] = np.float32(0.1)
    others = [c for c in range(views) if c not in (0, partner)]
    K[np.ix_(others, np.flatnonzero(far))] = K[np.ix_(others, np.flatnonzero(far))] * np.float32([1.0, 1.0, 0.0])
    K[0, far, 2] = K[partner, far, 2] = np.float32(0.9)
    if views >= 3:
        twin = (f % rare == 3) & (j < 4)
        K[1:-1, twin, 2] = np.float32(0.0)
        K[0, twin, 2] = K[-1, twin, 2] = np.float32(0.9)
        K[-1, twin, :2] = K[0, twin, :2]
    return np.ascontiguousarray(K), np.ascontiguousarray(cams), X


def holds_every_case(want, views):
    """What the tests that rely on a bundle of frames >= 15 and views >= 3 assert of the restatement's result, so that none passes on NaN alone."""
    return (set(np.unique(want["state"]).tolist()) == {OK, TOO_FEW, DEGENERATE, BEHIND} and set(np.unique(want["used"]).tolist()) == set(range(views + 1))
            and 2 * int((want["state"] == OK).sum()) >= len(want["state"]) and bool(np.isfinite(want["points"][want["state"] == OK]).all())
            and bool(np.isnan(want["points"][want["state"] != OK]).all()))
