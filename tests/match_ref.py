"""Shared by tests/test_match_cpu.py, tests/test_match_host_cpu.py, tests/test_gpu_match.py and tools/match_bench.py (not a test): the two rules of
include/kasf.h's kasf_match_pair_costs / kasf_match_groups in numpy -- fp64, one numpy operation per rounded operation of the rule, the sums in the rule's
order, fp32 rounding at the stores only -- with a port of csrc/assignment.h's augmenting-path walk, lane by lane, so that ties resolve as they do on the
device; and the generator of the tests' synthetic scene.  The text differs from the kernel's on purpose."""
import numpy as np

from tests.triangulate_ref import FMAX, HUGE, LENS, LIMIT, NAN32, _undistort64, project, ring, same_bits  # noqa: F401

TILE = 256                     # frames per tile of the summation order
PARALLEL = 1e-10
BIG = 1e9
DEFAULTS = dict(min_score=0.3, weighted=True, cap=50.0, min_samples=None, undistort_iterations=5)


def rays_np(K, cameras, min_score=0.3, undistort_iterations=5):
    """Step 1 over K [C,P,N,J,3] fp32, cameras [C,21] fp32 -> (usable [C,P,S] bool, d [3][C,P,S], score [C,P,S], o [3][C], f [C]) in fp64, S = N * J."""
    K = np.ascontiguousarray(K, np.float32)
    C, P, N, J = K.shape[:4]
    K = K.reshape(C, P, N * J, 3)
    cam32 = np.asarray(cameras, np.float32)
    with np.errstate(all="ignore"):
        use = (np.abs(K[..., :2]) <= LIMIT).all(-1) & (K[..., 2] >= np.float32(min_score)) & (np.abs(cam32) <= FMAX).all(-1)[:, None, None]
        cam = cam32.astype(np.float64)
        x, y = _undistort64(cam[:, None, None, :], K[..., 0].astype(np.float64), K[..., 1].astype(np.float64), undistort_iterations)
        R, t = cam[:, 9:18], cam[:, 18:21]
        d = [R[:, k, None, None] * x + R[:, 3 + k, None, None] * y + R[:, 6 + k, None, None] for k in range(3)]
        o = [0.0 - (R[:, k] * t[:, 0] + R[:, 3 + k] * t[:, 1] + R[:, 6 + k] * t[:, 2]) for k in range(3)]
        f = 0.5 * (cam[:, 0] + cam[:, 1])
    return use, d, K[..., 2].astype(np.float64), o, f


def pair_costs_np(K, cameras, min_score=0.3, weighted=True, cap=50.0, min_samples=None, undistort_iterations=5):
    """The pair rule -> (cost [C,C,P,P] fp32, samples [C,C,P,P] int32)."""
    C, P, N, J = np.shape(K)[:4]
    min_samples = 2 * J if min_samples is None else min_samples
    use, d, score, o, f = rays_np(K, cameras, min_score, undistort_iterations)
    cap = np.float64(np.float32(cap))
    cost = np.full((C, C, P, P), np.inf, np.float32)
    samples = np.zeros((C, C, P, P), np.int32)
    with np.errstate(all="ignore"):
        for a in range(C):
            for b in range(a + 1, C):
                A = [d[k][a][:, None, :] for k in range(3)]             # [P,1,S]
                B = [d[k][b][None, :, :] for k in range(3)]             # [1,P,S]
                w = [o[k][a] - o[k][b] for k in range(3)]
                aa = A[0] * A[0] + A[1] * A[1] + A[2] * A[2]
                bb = B[0] * B[0] + B[1] * B[1] + B[2] * B[2]
                ab = A[0] * B[0] + A[1] * B[1] + A[2] * B[2]
                da = A[0] * w[0] + A[1] * w[1] + A[2] * w[2]
                db = B[0] * w[0] + B[1] * w[1] + B[2] * w[2]
                det = aa * bb - ab * ab
                s = (ab * db - bb * da) / det
                t = (aa * db - ab * da) / det
                g = [(o[k][a] + s * A[k]) - (o[k][b] + t * B[k]) for k in range(3)]
                gap = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
                e = 0.5 * gap * (f[a] / s + f[b] / t)
                ok = (use[a][:, None, :] & use[b][None, :, :] & (det > PARALLEL * (aa * bb)) & (s > 0.0) & (t > 0.0) & (s <= HUGE) & (t <= HUGE)
                      & (np.abs(e) <= HUGE))
                wt = score[a][:, None, :] * score[b][None, :, :] if weighted else np.ones_like(e)
                term = wt * np.where(e < cap, e, cap)
                num, den, cnt = np.zeros((P, P)), np.zeros((P, P)), np.zeros((P, P), np.int64)
                for first in range(0, N, TILE):                         # a tile's sums from 0, sample by sample; the pair's sums take them in order
                    tn, td = np.zeros((P, P)), np.zeros((P, P))
                    for i in range(first * J, min(first + TILE, N) * J):
                        tn = np.where(ok[:, :, i], tn + term[:, :, i], tn)
                        td = np.where(ok[:, :, i], td + wt[:, :, i], td)
                    num, den = num + tn, den + td
                cnt = ok.sum(-1)
                c32 = np.where(cnt >= min_samples, (num / den).astype(np.float32), np.float32(np.inf)).astype(np.float32)
                cost[a, b], samples[a, b] = c32, cnt
                cost[b, a], samples[b, a] = c32.T, cnt.T
    return cost, samples


def assign_np(M):
    """csrc/assignment.h's walk over M [na, nb] fp64, 64 lanes as arrays -> (b_of_a [na], a_of_b [nb]), -1 for none."""
    na, nb = M.shape
    tr = na > nb
    nr, nc = (nb, na) if tr else (na, nb)
    cost = M.T if tr else M                                             # cost[row, column]
    lanes = np.arange(64)
    u, v = np.zeros(64), np.zeros(64)
    col4row, row4col = np.full(64, -1), np.full(64, -1)
    for cur in range(nr):
        spc, path = np.full(64, np.inf), np.full(64, -1)
        sc, sr = np.zeros(64, bool), np.zeros(64, bool)
        minval, i, sink = 0.0, cur, -1
        for _ in range(65):
            if sink >= 0:
                break
            sr[i] = True
            act = (lanes < nc) & ~sc
            c = np.zeros(64)
            c[:nc] = cost[i, :nc]
            r = minval + c - u[i] - v
            better = act & (r < spc)
            spc, path = np.where(better, r, spc), np.where(better, i, path)
            bv = np.where(act, spc, np.inf)
            bk = np.where(act, np.where(row4col >= 0, 64, 0), 128) + lanes
            j = int(np.lexsort((bk, bv))[0])                            # the least (value, key)
            if bk[j] >= 128:
                break
            minval = bv[j]
            if row4col[j] < 0:
                sink = j
            else:
                i = int(row4col[j])
            sc[j] = True
        if sink < 0:
            break
        sp = spc[np.where(col4row < 0, 0, col4row)]
        u = np.where(lanes == cur, u + minval, np.where(sr, u + (minval - sp), u))
        v = np.where(sc, v - (minval - spc), v)
        j = sink
        while True:
            ii = int(path[j])
            row4col[j] = ii
            col4row[ii], j = j, int(col4row[ii])
            if ii == cur:
                break
    a_of_b, b_of_a = (col4row, row4col) if tr else (row4col, col4row)
    return b_of_a[:na].copy(), a_of_b[:nb].copy()


def groups_np(cost, samples, max_cost=15.0, max_groups=None):
    """The grouping rule over cost fp32 and samples int32 [C,C,P,P] -> dict(group [C,P], members [G,C], views [G] int32, group_cost [G] fp32, count, dropped)."""
    cost, samples = np.asarray(cost, np.float32), np.asarray(samples, np.int32)
    C, P = cost.shape[0], cost.shape[2]
    G = min(64, 2 * P) if max_groups is None else max_groups
    max_cost = np.float64(np.float32(max_cost))
    group, members = np.full((C, P), -1, np.int32), np.full((G, C), -1, np.int32)
    views, accepted, cost_sum = np.zeros(G, np.int32), np.zeros(G, np.int64), np.zeros(G)
    count = dropped = 0
    for c in range(C):
        others = [m for m in range(C) if m != c]
        rows = [q for q in range(P) if (samples[c][others, q, :] > 0).any()]
        grp = {}
        if count > 0 and rows:
            M = np.zeros((len(rows), count))
            for k, q in enumerate(rows):
                for g in range(count):
                    num = den = 0.0
                    for m in range(c):
                        r = members[g, m]
                        if r >= 0 and np.abs(cost[m, c, r, q]) <= FMAX and samples[m, c, r, q] > 0:
                            num = num + float(samples[m, c, r, q]) * float(cost[m, c, r, q])
                            den = den + float(samples[m, c, r, q])
                    M[k, g] = num / den if den > 0.0 else BIG
            g_of_k, _ = assign_np(M)
            for k, g in enumerate(g_of_k):
                if g >= 0 and not (M[k, g] >= BIG or M[k, g] > max_cost):
                    grp[k] = int(g)
                    views[g] += 1
                    accepted[g] += 1
                    cost_sum[g] = cost_sum[g] + M[k, g]
        for k, q in enumerate(rows):
            if k not in grp:
                if count < G:
                    grp[k] = count
                    views[count] = 1
                    count += 1
                else:
                    dropped += 1
        for k, g in grp.items():
            group[c, rows[k]] = g
            members[g, c] = rows[k]
    with np.errstate(all="ignore"):
        group_cost = np.where(accepted > 0, (cost_sum / accepted).astype(np.float32), NAN32).astype(np.float32)
    return dict(group=group, members=members, views=views, group_cost=group_cost, count=np.int32(count), dropped=np.int32(dropped))


# ---- the synthetic scene ----

def scene(frames=24, cameras=5, players=6, joints=17, seed=0, noise=1.0, pad=1, lifetimes=False):
    """`players` players seen by a ring of `cameras` cameras (camera 1 has a lens with distortion) over `frames` synchronised frames, a pixel of noise, scores
    in [0.5, 1]; every camera lists the players in its own order, with `pad` empty rows (score 0) among them.  With 5 or more players the last but one is
    absent from cameras 1 and 3 and the last is seen by camera 2 alone.  lifetimes: player i is tracked from frame 3 i to frame `frames` - 2 i only.
    -> (K [cameras, players + pad, frames, joints, 3] fp32, cams [cameras, 21] fp32, X [players, frames, joints, 3] fp64, row [cameras, players]: the row of
    player i in camera c, or -1)."""
    rng = np.random.default_rng(4000 + seed)
    cams = ring(cameras, rng)
    if cameras > 1:
        cams[1, 4:9] = LENS
    start = np.stack([rng.uniform(-4.0, 4.0, players), rng.uniform(-4.0, 4.0, players), rng.uniform(0.9, 1.1, players)], 1)
    for i in range(players if players <= 8 else 0):                     # up to 8 players stand apart: at least 1.5 m between any two starts
        while i and np.linalg.norm(start[:i, :2] - start[i, :2], axis=1).min() < 1.5:
            start[i, :2] = rng.uniform(-4.0, 4.0, 2)
    step = np.concatenate([rng.uniform(-0.02, 0.02, (players, 2)), np.zeros((players, 1))], 1)
    body = rng.uniform(-0.5, 0.5, (players, 1, joints, 3)) * [0.5, 0.5, 1.6]
    X = start[:, None, None, :] + step[:, None, None, :] * np.arange(frames)[None, :, None, None] + body
    P = players + pad
    K = np.zeros((cameras, P, frames, joints, 3), np.float32)
    row = np.full((cameras, players), -1)
    for c in range(cameras):
        order = rng.permutation(P)
        for i in range(players):
            if players >= 5 and ((i == players - 2 and c in (1, 3)) or (i == players - 1 and c != 2 % cameras)):
                continue
            row[c, i] = order[i]
            uv = project(X[i].reshape(-1, 3), cams[c:c + 1])[0] + rng.normal(0.0, noise, (frames * joints, 2))
            K[c, order[i]] = np.concatenate([uv, rng.uniform(0.5, 1.0, (frames * joints, 1))], -1).astype(np.float32).reshape(frames, joints, 3)
            if lifetimes:
                K[c, order[i], :min(3 * i, frames), :, 2] = 0.0
                K[c, order[i], max(frames - 2 * i, 0):, :, 2] = 0.0
    return K, cams, X, row


def truth_partition(row):
    """row [cameras, players] -> the set of groups, each a frozenset of (camera, row), that the truth asks for."""
    return {frozenset((c, int(r)) for c, r in enumerate(col) if r >= 0) for col in row.T if (col >= 0).any()}


def partition_of(members):
    """members [G, cameras] -> the set of the opened groups as frozensets of (camera, row)."""
    return {frozenset((c, int(r)) for c, r in enumerate(g) if r >= 0) for g in members if (g >= 0).any()}
