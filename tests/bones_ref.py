"""Shared by tests/test_bones_cpu.py, tests/test_bones_host_cpu.py and tests/test_gpu_bones.py (not a test): the constant-limb-length rule of include/kasf.h
(kasf_bone_median / _apply / _push / _tracked) in numpy, in fp32 -- one numpy operation per rounded operation of the rule, on numpy scalars or arrays of one
type, never a Python float -- and the cases the three files run.  The row rule of the tracked entry is tests/tracked_ref.py's ``tracked_front_np``."""
import numpy as np

from tests.tracked_ref import tracked_front_np

PARENTS = (0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
CHILDREN = tuple(range(1, 17))
PARTNERS = ((0, 3), (1, 4), (2, 5), (10, 13), (11, 14), (12, 15))
F32 = np.float32


def frame_lengths(x):
    """x [..., 17, 3] fp32 -> (v [..., 16, 3], l [..., 16], usable [..., 16]): rule 1, without the frame's own usability."""
    with np.errstate(all="ignore"):
        v = x[..., CHILDREN, :] - x[..., PARENTS, :]
        sq = v * v
        l = np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])
    return v, l, np.isfinite(l) & (l > 0)


def frames_usable(x):
    return np.isfinite(x).all(axis=(-1, -2))


def lower_median(values):
    """The element of rank (n - 1) // 2 of the values in ascending order -> (L, n); (0, 0) for none."""
    n = len(values)
    return (np.sort(values)[(n - 1) // 2], n) if n else (F32(0), 0)


def median_np(x, offsets):
    """kasf_bone_median: x [N,17,3] fp32, offsets [P+1] -> (lengths [P,16] fp32, counts [P,16] int32)."""
    P = len(offsets) - 1
    _, l, ok = frame_lengths(x)
    ok = ok & frames_usable(x)[:, None]
    L, cnt = np.zeros((P, 16), F32), np.zeros((P, 16), np.int32)
    for p in range(P):
        a, b = int(offsets[p]), int(offsets[p + 1])
        for k in range(16):
            L[p, k], cnt[p, k] = lower_median(l[a:b, k][ok[a:b, k]])
    return L, cnt


def median_of_scratch_np(scratch, offsets):
    """The select alone: scratch [16,N] fp32 where a value that is not positive and finite does not count -> (lengths, counts)."""
    P = len(offsets) - 1
    L, cnt = np.zeros((P, 16), F32), np.zeros((P, 16), np.int32)
    for p in range(P):
        for k in range(16):
            s = scratch[k, int(offsets[p]):int(offsets[p + 1])]
            L[p, k], cnt[p, k] = lower_median(s[np.isfinite(s) & (s > 0)])
    return L, cnt


def symmetric_np(L):
    """Rule 3 over a table [..., 16] -> a new table."""
    out = L.copy()
    for a, b in PARTNERS:
        La, Lb = L[..., a], L[..., b]
        with np.errstate(all="ignore"):
            mean = (La + Lb) * F32(0.5)
        m = np.where((La > 0) & (Lb > 0), mean, np.where(La > 0, La, np.where(Lb > 0, Lb, F32(0)))).astype(F32)
        out[..., a], out[..., b] = m, m
    return out


def walk_np(x, L):
    """Rule 4 for one frame x [17,3] fp32 and a table L [16] fp32 (already symmetric if wanted) -> y [17,3]; an unusable frame is returned as it is."""
    if not np.isfinite(x).all():
        return x.copy()
    v, l, ok = frame_lengths(x)
    y = x.copy()
    with np.errstate(all="ignore"):
        for k in range(16):
            c, p = k + 1, PARENTS[k]
            if L[k] > 0 and ok[k]:
                s = L[k] / l[k]
                y[c] = y[p] + v[k] * s
            else:
                y[c] = y[p] + v[k]
    return y


def apply_np(x, offsets, L, symmetric):
    """kasf_bone_apply: x [N,17,3]; L [P,16] with offsets, or [16] for every frame -> out [N,17,3]."""
    L = symmetric_np(L) if symmetric else L
    out = x.copy()
    if L.ndim == 1:
        for f in range(len(x)):
            out[f] = walk_np(x[f], L)
        return out
    for p in range(len(offsets) - 1):
        for f in range(int(offsets[p]), int(offsets[p + 1])):
            out[f] = walk_np(x[f], L[p])
    return out


def apply_arrays_np(x, offsets, L, symmetric):
    """apply_np once more, over all frames at once with masks (what a caller without the device op would write): the same bits."""
    L = symmetric_np(L) if symmetric else L
    if L.ndim == 2:
        Lf = np.zeros((len(x), 16), F32)
        for p in range(len(offsets) - 1):
            Lf[int(offsets[p]):int(offsets[p + 1])] = L[p]
    else:
        Lf = np.broadcast_to(L, (len(x), 16))
    v, l, ok = frame_lengths(x)
    scale = ok & (Lf > 0)
    y = x.copy()
    with np.errstate(all="ignore"):
        s = np.where(scale, Lf / np.where(scale, l, F32(1)), F32(1)).astype(F32)
        for k in range(16):
            w = np.where(scale[:, k, None], v[:, k] * s[:, k, None], v[:, k])
            y[:, k + 1] = y[:, PARENTS[k]] + w
    bad = ~frames_usable(x)
    y[bad] = x[bad]
    return y


def fix_np(x, offsets, symmetric=False):
    L, _ = median_np(x, offsets)
    return apply_np(x, offsets, L, symmetric)


def new_state(S, fill=0.0):
    """len [S,16] (any initial value: never read while cnt is 0), cnt [S,16] zeros, owner [S] zeros; count / ring serve tracked_front_np only."""
    return dict(len=np.full((S, 16), fill, F32), cnt=np.zeros((S, 16), np.int32), owner=np.zeros(S, np.int32), count=np.zeros(S, np.int64),
                ring=np.zeros((S, 1, 1, 1), F32))


def live_row_np(state, x, g, window, symmetric, restart=False):
    """Rule 5 for one row x [17,3] and slot g, the state updated in place -> y [17,3]."""
    if restart:
        state["cnt"][g] = 0
    if not np.isfinite(x).all():
        return x.copy()
    _, l, ok = frame_lengths(x)
    ln, cnt = state["len"][g], state["cnt"][g]
    with np.errstate(all="ignore"):
        for k in range(16):
            if not ok[k]:
                continue
            d = min(int(cnt[k]) + 1, window)
            if cnt[k] == 0:
                ln[k] = l[k]
            else:
                e = l[k] - ln[k]
                e = e / F32(d)
                ln[k] = ln[k] + e
            cnt[k] = d
    L = np.where(cnt > 0, ln, F32(0)).astype(F32)
    return walk_np(x, symmetric_np(L) if symmetric else L)


def push_np(state, x, slots, window, symmetric):
    """kasf_bone_push: x [K,17,3], slots [K] or None -> out; an id outside [0, S) copies through."""
    S = state["len"].shape[0]
    out = x.copy()
    for i in range(len(x)):
        g = i if slots is None else int(slots[i])
        if 0 <= g < S:
            out[i] = live_row_np(state, x[i], g, window, symmetric)
    return out


def tracked_np(state, x, track_arrays, rows, R, window, symmetric):
    """kasf_bone_tracked: x [B*R,17,3]; the rows resolved by tracked_front_np (which moves owner / count) -> (out, row_slot, reset, why)."""
    row_slot, reset, why = tracked_front_np(state, track_arrays, rows, R)
    out = x.copy()
    for row in range(len(x)):
        g = int(row_slot[row])
        if g >= 0:
            out[row] = live_row_np(state, x[row], g, window, symmetric, restart=bool(reset[row]))
    return out, row_slot, reset, why


EPS = 2.0 ** -24


def length_excess(y, L, scaled):
    """How far the bones of y [..., 17, 3] (fp32, looked at in fp64) are from the table L [..., 16], over the bound of tests/test_bones_cpu.py's docstring,
    4 eps L + 2 sqrt(3) eps max(|y_p|inf, |y_c|inf); `scaled` [..., 16] marks the bones the walk scaled.  -> the largest (error - bound), <= 0 when it holds."""
    y = y.astype(np.float64)
    yc, yp = y[..., CHILDREN, :], y[..., PARENTS, :]
    got = np.linalg.norm(yc - yp, axis=-1)
    bound = 4 * EPS * L + 2 * np.sqrt(3) * EPS * np.maximum(np.abs(yc).max(-1), np.abs(yp).max(-1))
    return float(np.where(scaled, np.abs(got - L) - bound, -np.inf).max())


# ---- cases ----
SKELETON = np.array([[0, 0, 0], [-0.13, 0, 0], [-0.13, -0.45, 0.02], [-0.13, -0.9, 0], [0.13, 0, 0], [0.14, -0.44, 0.02], [0.13, -0.88, 0], [0, 0.25, 0.02],
                     [0, 0.5, 0], [0, 0.6, 0.03], [0, 0.72, 0.02], [0.18, 0.48, 0], [0.2, 0.2, 0.03], [0.21, -0.05, 0.1], [-0.18, 0.48, 0], [-0.2, 0.21, 0.03],
                     [-0.2, -0.03, 0.1]], np.float64)        # a standing figure in metres, left and right limbs a little different


def synthetic_track(n, noise, seed=0, dtype=F32):
    """SKELETON under a random rotation and translation per frame plus Gaussian joint noise of `noise` metres -> [n,17,3]."""
    g = np.random.default_rng(seed)
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    rot = np.stack([np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)], -1),
                    np.stack([2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)], -1),
                    np.stack([2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)], -1)], 1)
    x = np.einsum("nij,kj->nki", rot, SKELETON) + g.normal(size=(n, 1, 3)) + g.normal(size=(n, 17, 3)) * noise
    return x.astype(dtype)


def true_lengths():
    return np.linalg.norm(SKELETON[list(CHILDREN)] - SKELETON[list(PARENTS)], axis=1)


def limb_var(x):
    """loss_limb_var_calc's definition over one track x [n,17,3], in fp64: the unbiased variance of every bone's length over time, averaged over the bones."""
    x = x.astype(np.float64)
    l = np.linalg.norm(x[:, CHILDREN] - x[:, PARENTS], axis=-1)
    return float(np.var(l, axis=0, ddof=1).mean())


MEDIAN_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 300)


def median_tracks(seed=5):
    """Packed poses and offsets for the median cases: tracks of MEDIAN_LENGTHS frames (the empty one between two others), then a track of all-equal frames, one
    of heavy ties, one with zero-length bones, one with a NaN or an infinity in one joint of some frames, and one with no usable frame."""
    g = np.random.default_rng(seed)
    tracks = [synthetic_track(n, 0.02, seed + i) for i, n in enumerate((1, 0, 2, 3, 63, 64, 65, 300))]
    tracks.append(np.repeat(synthetic_track(1, 0.0, seed + 20), 70, axis=0))                                 # all equal
    ties = synthetic_track(4, 0.02, seed + 21)
    tracks.append(ties[g.integers(0, 4, 90)])                                                                # four distinct frames, many times each
    zero = synthetic_track(40, 0.02, seed + 22)
    zero[:, 2] = zero[:, 1]                                                                                  # bone 1 has length 0 in every frame
    zero[::3, 16] = zero[::3, 15]                                                                            # bone 15 in every third
    tracks.append(zero)
    bad = synthetic_track(50, 0.02, seed + 23)
    bad[::4, 5, 1] = np.nan
    bad[1::7, 12, 2] = np.inf
    bad[2::9, 0, 0] = -np.inf
    tracks.append(bad)
    none = synthetic_track(9, 0.02, seed + 24)
    none[:, 3, 0] = np.nan
    tracks.append(none)
    huge = synthetic_track(12, 0.02, seed + 25) * F32(1e30)                                                  # squares overflow: no usable length, frames finite
    tiny = synthetic_track(12, 0.02, seed + 26) * F32(1e-21)                                                 # squares are denormal or 0
    tracks += [huge, tiny]
    off = np.cumsum([0] + [len(t) for t in tracks]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(tracks)), off


def select_scratch(seed=7):
    """The select alone: scratch [16,N] of bit patterns no pose can produce as well -- 1e-30 .. 1e30, denormals, 0, -1, NaN, inf -- and offsets."""
    g = np.random.default_rng(seed)
    lengths = (0, 1, 2, 3, 63, 64, 65, 300, 0, 257)
    off = np.cumsum([0] + list(lengths)).astype(np.int64)
    N = int(off[-1])
    s = (10.0 ** g.uniform(-30, 30, (16, N))).astype(F32)
    s[1] = F32(2.5)                                                                                          # all equal
    s[2] = g.integers(1, 4, N).astype(F32)                                                                   # heavy ties
    s[3] = (g.integers(1, 2 ** 23, N).astype(np.uint32)).view(F32)                                           # denormals only
    s[4, ::2] = (g.integers(1, 2 ** 23, (N + 1) // 2).astype(np.uint32)).view(F32)                           # denormals among normals
    s[5, ::3] = 0
    s[6] = 0                                                                                                 # nothing usable
    s[7, ::5], s[7, 1::5], s[7, 2::5] = np.nan, np.inf, -1.0
    s[8] = np.sort(s[8])
    s[9] = np.sort(s[9])[::-1]
    s[10] = np.nextafter(F32(1), F32(2)) * (g.integers(0, 2, N).astype(F32)) + F32(1)                        # two neighbours in the last bit... and 1
    s[11] = F32(3.4028235e38)
    return np.ascontiguousarray(s), off


def live_rows(tick, n_rows, seed=0):
    """Rows [n_rows,17,3] of a live pipeline: a figure with noise per row, a NaN or an infinity or a zero-length bone put in now and then."""
    x = synthetic_track(n_rows, 0.03, 1000 * seed + tick)
    if tick % 5 == 3:
        x[0, 4, 1] = np.nan
    if tick % 7 == 4:
        x[-1, 16, 2] = np.inf
    if tick % 4 == 2:
        x[-1, 6] = x[-1, 5]                                                                                  # bone 5 has length 0
    return x
