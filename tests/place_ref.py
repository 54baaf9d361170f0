"""Shared by tests/test_place_cpu.py, tests/test_place_host_cpu.py, tests/test_gpu_place.py and tools/place_bench.py (not a test): the rule of include/kasf.h's
kasf_pose_place in numpy -- fp64, one numpy operation per rounded operation of the rule, joints and bones in ascending order, fp32 rounding at the stores
only -- and the generators of its tests: a synthetic skeleton, a pinhole projection, scenes of players in front of a camera and a ``bundle`` of frames that
contains every state.

The text differs from the kernel's on purpose: it works on all frames at once, a joint that is not usable is masked out of a sum where the kernel skips it, and
the state is read off the header's list at the end where the kernel carries a flag."""
import numpy as np

LIMIT = np.float32(1e12)
PARENTS = (0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)         # bone b joins joint b + 1 to PARENTS[b] (kasf.h, kasf_bone_median)
PIVOT = 1e-9
HUGE = np.finfo(np.float64).max
PLACED, TOO_FEW, DEGENERATE, UNUSABLE = 0, 1, 2, 3
NAN32 = np.array([0x7fc00000], np.uint32).view(np.float32)[0]
# the sixteen bone lengths of a 1.7 m person, metres: right hip, thigh, shin, left hip, thigh, shin, spine, thorax, neck, head, left shoulder, upper arm,
# forearm, right shoulder, upper arm, forearm
BONES_170 = np.array([0.13, 0.45, 0.44, 0.13, 0.45, 0.44, 0.24, 0.26, 0.11, 0.12, 0.15, 0.29, 0.25, 0.15, 0.29, 0.25], np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def usable_np(P, K, min_score):
    """Step 1 over P, K [N,17,3] fp32 -> bool [N,17]."""
    with np.errstate(all="ignore"):
        return (np.abs(K[..., :2]) <= LIMIT).all(-1) & (K[..., 2] >= np.float32(min_score)) & (np.abs(P) <= np.finfo(np.float32).max).all(-1)


def place_np(P, K, camera, lengths=None, min_score=0.3, weighted=True, iterations=4, delta=3.0, min_joints=4):
    """The rule over P, K [N,17,3] fp32, camera [4] or [N,4] fp32, lengths None, [16] or [N,16] fp32 ->
    dict(poses [N,17,3], root [N,3], residual [N], scale [N], all fp32, and state [N] uint8)."""
    P, K = np.ascontiguousarray(P, np.float32).reshape(-1, 17, 3), np.ascontiguousarray(K, np.float32).reshape(-1, 17, 3)
    N = len(P)
    cam = np.broadcast_to(np.asarray(camera, np.float32).reshape(-1, 4), (N, 4)).astype(np.float64)
    fx, fy, cx, cy = cam[:, 0], cam[:, 1], cam[:, 2], cam[:, 3]
    p64, k64 = P.astype(np.float64), K.astype(np.float64)
    use = usable_np(P, K, min_score)
    with np.errstate(all="ignore"):
        scale = np.ones(N)
        if lengths is not None:                                          # step 2
            L = np.broadcast_to(np.asarray(lengths, np.float32).reshape(-1, 16), (N, 16))
            sumL, sumP = np.zeros(N), np.zeros(N)
            for b in range(16):
                on = L[:, b] > 0
                d = p64[:, b + 1] - p64[:, PARENTS[b]]
                length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                sumL = np.where(on, sumL + L[:, b].astype(np.float64), sumL)
                sumP = np.where(on, sumP + length, sumP)
            scale = sumL / sumP
        ps = p64 * scale[:, None, None]
        d2 = np.float64(np.float32(delta)) * np.float64(np.float32(delta))
        w0 = k64[:, :, 2] if weighted else np.ones((N, 17))
        T = np.zeros((N, 3))
        bad = np.zeros(N, bool)

        def r2_at(j):                                                    # step 4's squared pixel distance of joint j at T, and whether it is in front
            X, Y, Z = ps[:, j, 0] + T[:, 0], ps[:, j, 1] + T[:, 1], ps[:, j, 2] + T[:, 2]
            du, dv = (fx * (X / Z) + cx) - k64[:, j, 0], (fy * (Y / Z) + cy) - k64[:, j, 1]
            return du * du + dv * dv, Z > 0.0

        for it in range(iterations + 1):                                 # steps 3 and 4
            S, Sx, Sy, Sq, b0, b1, b2 = (np.zeros(N) for _ in range(7))
            for j in range(17):
                u = use[:, j]
                w = w0[:, j]
                if it > 0:
                    r2, front = r2_at(j)
                    bad |= u & ~front
                    w = w0[:, j] / (1.0 + r2 / d2)
                xh, yh = (k64[:, j, 0] - cx) / fx, (k64[:, j, 1] - cy) / fy
                q1, q2 = xh * ps[:, j, 2] - ps[:, j, 0], yh * ps[:, j, 2] - ps[:, j, 1]
                S = np.where(u, S + w, S)
                Sx = np.where(u, Sx + w * xh, Sx)
                Sy = np.where(u, Sy + w * yh, Sy)
                Sq = np.where(u, Sq + w * (xh * xh + yh * yh), Sq)
                b0 = np.where(u, b0 + w * q1, b0)
                b1 = np.where(u, b1 + w * q2, b1)
                b2 = np.where(u, b2 + w * (xh * q1 + yh * q2), b2)
            D = Sq - (Sx * Sx + Sy * Sy) / S
            bad |= ~(S > 0.0) | ~(D > PIVOT * Sq)
            Tz = ((Sx * b0 + Sy * b1) / S - b2) / D
            Tx, Ty = (b0 + Sx * Tz) / S, (b1 + Sy * Tz) / S
            T = np.stack([Tx, Ty, Tz], 1)
            bad |= ~(np.abs(T) <= HUGE).all(1)
        num, den = np.zeros(N), np.zeros(N)                              # step 5
        for j in range(17):
            u = use[:, j]
            r2, front = r2_at(j)
            bad |= u & ~front
            num = np.where(u, num + w0[:, j] * r2, num)
            den = np.where(u, den + w0[:, j], den)
        state = np.where(use.sum(1) < min_joints, TOO_FEW, np.where((scale > 0.0) & (scale <= HUGE), np.where(bad, DEGENERATE, PLACED), UNUSABLE)).astype(np.uint8)
        ok = state == PLACED
        out = np.where(ok[:, None, None], (ps + T[:, None, :]).astype(np.float32), NAN32)
        root = np.where(ok[:, None], T.astype(np.float32), NAN32)
        residual = np.where(ok, np.sqrt(num / den).astype(np.float32), NAN32)
    return dict(poses=out, root=root, residual=residual, scale=scale.astype(np.float32), state=state)


# ---- generators ----

def skeleton(rng, n, bones=BONES_170):
    """n root-relative skeletons [n,17,3] fp32 with the given bone lengths and random bone directions; joint 0 at the origin."""
    P = np.zeros((n, 17, 3))
    for b in range(16):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        P[:, b + 1] = P[:, PARENTS[b]] + float(bones[b]) * d
    return P.astype(np.float32)


def project(X, camera):
    """Pinhole: X [..,3] -> pixels [..,2] in fp64; camera [4] or [..,4] broadcast over the joints."""
    c = np.asarray(camera, np.float64)
    c = c.reshape(c.shape[:-1] + (1,) * (X.ndim - c.ndim) + (4,)) if c.ndim > 1 else c
    return np.stack([c[..., 0] * X[..., 0] / X[..., 2] + c[..., 2], c[..., 1] * X[..., 1] / X[..., 2] + c[..., 3]], -1)


def scene(rng, n, f=1500.0, depth=(4.0, 40.0), size=(1920.0, 1080.0), camera=None):
    """n players in front of a camera: (poses [n,17,3] fp32 root-relative metres, T_true [n,3] fp64, keypoints [n,17,3] fp32, camera [4] fp32).  The keypoints
    are the fp32 poses plus T_true projected in fp64 and rounded to fp32; the scores are drawn from [0.5, 1]."""
    camera = np.array([f, f, size[0] / 2, size[1] / 2], np.float32) if camera is None else np.asarray(camera, np.float32)
    P = skeleton(rng, n)
    z = rng.uniform(depth[0], depth[1], n)
    cam = np.broadcast_to(camera.reshape(-1, 4), (n, 4)).astype(np.float64)
    T = np.stack([rng.uniform(-0.3, 0.3, n) * size[0] / cam[:, 0] * z, rng.uniform(-0.3, 0.3, n) * size[1] / cam[:, 1] * z, z], 1)
    uv = project(P.astype(np.float64) + T[:, None, :], camera)
    K = np.concatenate([uv, rng.uniform(0.5, 1.0, (n, 17, 1))], -1).astype(np.float32)
    return P, T, K, camera


def bundle(n, seed=0, table=True, per_frame=False):
    """n frames that hold every state (state 3 needs ``table``): (poses, keypoints, camera, lengths or None).  Poses are in an arbitrary unit per frame when a
    table is given; by frame index modulo 11: 3 too few joints, 5 all keypoints in one point, 7 a pose behind the camera, 9 a NaN pose value; everywhere a pixel
    of noise, some low scores, a NaN keypoint and an outlier now and then.  ``per_frame``: camera [n,4] and lengths [n,16]."""
    rng = np.random.default_rng(1000 + seed)
    P, T, K, camera = scene(rng, n)
    if per_frame:
        camera = (camera[None, :] * rng.uniform(0.8, 1.25, (n, 1)).astype(np.float32)).astype(np.float32)
        K[..., :2] = project(P.astype(np.float64) + T[:, None, :], camera).astype(np.float32)
    i = np.arange(n)
    behind = i % 11 == 7
    if behind.any():
        Tb = T[behind] * np.array([1.0, 1.0, -1.0])
        K[behind, :, :2] = project(P[behind].astype(np.float64) + Tb[:, None, :], camera[behind] if per_frame else camera).astype(np.float32)
    K[..., :2] += rng.normal(0.0, 1.0, (n, 17, 2)).astype(np.float32)
    low = rng.random((n, 17)) < 0.1
    K[..., 2] = np.where(low, rng.uniform(0.0, 0.29, (n, 17)), K[..., 2]).astype(np.float32)
    K[i % 11 == 3, 3:, 2] = np.float32(0.1)
    K[i % 11 == 5, :, :2] = K[i % 11 == 5, :1, :2]
    K[i % 13 == 1, 4, 0] = np.nan
    K[i % 13 == 6, 16, :2] += np.float32(150.0)
    lengths = None
    if table:
        P = (P * rng.uniform(0.05, 400.0, (n, 1, 1)).astype(np.float32)).astype(np.float32)
        lengths = BONES_170.copy()
        lengths[9] = 0.0                                                 # skip the head
        if per_frame:
            lengths = (lengths[None, :] * rng.uniform(0.9, 1.1, (n, 1)).astype(np.float32)).astype(np.float32)
    P[i % 11 == 9, 12, 1] = np.nan
    return np.ascontiguousarray(P), np.ascontiguousarray(K), camera, lengths
