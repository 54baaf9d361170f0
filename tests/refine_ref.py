"""Shared by tests/test_refine_cpu.py, tests/test_refine_host_cpu.py, tests/test_gpu_refine.py and tools/refine_bench.py (not a test): the rule of
include/kasf.h's kasf_tracks_refine in numpy, in fp32 -- one numpy operation per rounded operation of the rule, on arrays of one type, never a Python float --
and in fp64 (``ft=np.float64``: the same statements on the upcast inputs and weights).

The text differs from the kernel's on purpose: the neighbours a and b come from running indices over the whole track (no bounded search), the states from the
header's table as it is written, and the window sums walk k = -radius .. radius over every frame of a track at once, a frame taking part while |k| <= r."""
import numpy as np

LIMIT = np.float32(1e12)
MAX_GAP, MAX_RADIUS = 64, 32
USABLE, INTERPOLATED, HELD, LEFT = 0, 1, 2, 3


def weights(sigma, radius=None):
    """(w [33] fp32, radius): w[k] = float32(exp(-k^2 / (2 sigma^2))) in fp64 rounded once, zeros above radius; radius None -> min(32, ceil(3 sigma)); sigma None
    -> radius 0."""
    if sigma is None:
        sigma, radius = 1.0, 0
    if radius is None:
        radius = min(MAX_RADIUS, int(np.ceil(3.0 * sigma)))
    w = np.zeros(MAX_RADIUS + 1, np.float32)
    k = np.arange(radius + 1, dtype=np.float64)
    w[:radius + 1] = np.exp(-k * k / (2.0 * float(sigma) ** 2)).astype(np.float32)
    return w, int(radius)


def usable_np(x, C, has_score, min_score):
    """Step 1 over [n, J, Ct] -> bool [n, J]."""
    with np.errstate(all="ignore"):
        u = (np.abs(x[..., :C]) <= LIMIT).all(-1)                  # False for a NaN
        if has_score:
            u &= x[..., C] >= np.float32(min_score)
    return u


def fill_np(x, C, has_score, min_score, max_gap, ft=np.float32):
    """Step 2 for one track x [n, J, Ct] -> (y [n, J, C] of type ft, state [n, J] uint8); y of an unknown joint is the input."""
    n, J = x.shape[:2]
    u = usable_np(x, C, has_score, min_score)
    idx = np.arange(n)[:, None]
    a = np.full((n, J), -1, np.int64)                              # the nearest usable frame before, -1 for none
    b = np.full((n, J), n, np.int64)                               # the nearest after, n for none
    for f in range(1, n):
        a[f] = np.where(u[f - 1], f - 1, a[f - 1])
    for f in range(n - 2, -1, -1):
        b[f] = np.where(u[f + 1], f + 1, b[f + 1])
    has_a, has_b = a >= 0, b < n
    state = np.full((n, J), LEFT, np.uint8)
    interp = ~u & has_a & has_b & (b - a - 1 <= max_gap)
    lead = ~u & ~has_a & has_b & (b - 0 <= max_gap)
    trail = ~u & has_a & ~has_b & (n - 1 - a <= max_gap)
    state[u], state[interp], state[lead | trail] = USABLE, INTERPOLATED, HELD
    xs = x[..., :C].astype(ft)
    y = xs.copy()
    jj = np.broadcast_to(np.arange(J), (n, J))
    ac, bc = np.clip(a, 0, max(n - 1, 0)), np.clip(b, 0, max(n - 1, 0))
    if n:
        xa, xb = xs[ac, jj], xs[bc, jj]                            # [n, J, C]
        with np.errstate(all="ignore"):
            t = ((idx - a).astype(ft) / np.maximum(b - a, 1).astype(ft))[..., None]
            d = xb - xa
            d = d * t
            d = xa + d
        y[interp] = d[interp]
        y[lead] = xb[lead]
        y[trail] = xa[trail]
    return y, state


def smooth_np(y, state, w, radius, ft=np.float32):
    """Step 3 for one track: y [n, J, C], state [n, J] -> the smoothed values [n, J, C]; unknown joints keep y."""
    n = y.shape[0]
    known = state < LEFT
    f = np.arange(n)
    r = np.minimum(np.minimum(radius, f), n - 1 - f)               # [n]
    num, den = np.zeros(y.shape, ft), np.zeros(state.shape, ft)
    wt = w.astype(ft)
    for k in range(-radius, radius + 1):
        sel = f[r >= abs(k)]                                       # the frames whose window holds k; then 0 <= sel + k < n
        if sel.size == 0:
            continue
        m = sel + k
        take = known[m]                                            # [s, J]
        with np.errstate(all="ignore"):                            # an unknown joint may hold anything; it is not taken
            d = y[m] - y[sel]
            d = wt[abs(k)] * d
            s = num[sel] + d
        num[sel] = np.where(take[..., None], s, num[sel])
        den[sel] = np.where(take, den[sel] + wt[abs(k)], den[sel])
    out = y.copy()
    with np.errstate(all="ignore"):
        q = num / den[..., None]
        q = y + q
    out[known] = q[known]
    return out


def refine_np(x, offsets, has_score, min_score=0.3, max_gap=15, w=None, radius=0, ft=np.float32, filled=False):
    """kasf_tracks_refine: x [N, J, Ct] fp32 packed, offsets [P + 1] (clamped as the entry clamps them) -> (out [N, J, Ct] of type ft, state [N, J] uint8).
    Rows outside every track keep the NaN / 255 this starts from: "not written".  filled: the filled y instead of the smoothed output."""
    N, J, Ct = x.shape
    C = Ct - (1 if has_score else 0)
    out, state = np.full(x.shape, np.nan, ft), np.full((N, J), 255, np.uint8)
    if w is None:
        w = np.zeros(MAX_RADIUS + 1, np.float32)
        w[0] = 1
    for p in range(len(offsets) - 1):
        lo = int(np.clip(offsets[p], 0, N))
        hi = int(np.clip(offsets[p + 1], lo, N))
        if hi <= lo:
            continue
        xt = x[lo:hi]
        y, st = fill_np(xt, C, has_score, min_score, max_gap, ft)
        o = y if filled or radius == 0 else smooth_np(y, st, w, radius, ft)
        res = xt.astype(ft)                                        # the score, and every unknown joint bit for bit
        known = st < LEFT
        res[..., :C][known] = o[known]
        out[lo:hi], state[lo:hi] = res, st
    return out, state


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint64),
                                                                        b.view(np.uint32 if b.itemsize == 4 else np.uint64))


def synthetic_track(n=600, J=17, seed=0):
    """The sanity track: 60 px sinusoids at 0.5 Hz sampled at 30 fps around centres in [100, 640), 2 px of noise, about 11 % of the joint-frames in gaps of 1-10
    frames with 200 px outliers and scores below 0.3 -> (x [n, J, 3] fp32, truth [n, J, 2] fp64, gated [n, J] bool)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None, None] / 30.0
    centre = rng.uniform(100.0, 640.0, (1, J, 2))
    phase = rng.uniform(0.0, 2 * np.pi, (1, J, 2))
    truth = centre + 60.0 * np.sin(2 * np.pi * 0.5 * t + phase)
    xy = truth + rng.normal(0.0, 2.0, truth.shape)
    score = rng.uniform(0.5, 1.0, (n, J))
    gated = np.zeros((n, J), bool)
    for j in range(J):
        f = int(rng.integers(5, 40))
        while f < n - 12:
            g = int(rng.integers(1, 11))
            gated[f:f + g, j] = True
            f += g + int(rng.integers(20, 80))
    k = int(gated.sum())
    xy[gated] += rng.choice([-200.0, 200.0], (k, 2))
    score[gated] = rng.uniform(0.0, 0.29, k)
    return np.concatenate([xy, score[..., None]], -1).astype(np.float32), truth, gated


LONG = 300                                  # the long track starts at packed frame 0: the kernel's tiles of 64 frames cut it at 64, 128, 192, 256


def gate(x, C, score, frames, j):
    """Makes joint j unusable in `frames`: a low score where there is one, else a NaN."""
    if score:
        x[frames, j, C] = 0.1
    else:
        x[frames, j, C - 1] = np.nan


def bundle(J, C, score, seed=0, offsets="exact"):
    """(x [N, J, Ct] fp32, offsets int64 [P + 1]) for the kernel tests: one track of 300 frames from packed frame 0, so it crosses four tile edges, with about 30 %
    of its joints gated at random (tests/smooth_ref.rows_for) and runs placed on tile edges -- a gap of 9 across frame 64, gaps of 64 and of 65 frames between
    edges, a leading run of 71, a trailing run of 64 --, then 40 tracks of 0 - 5 frames inside one tile, then a track of 70 frames that crosses an edge off
    the grid, its first joint never usable.  offsets: "exact"; "clamped" (a first entry below 0 and a last one beyond N); "inner" (two rows in front of the first
    track and three behind the last belong to no track)."""
    from tests.smooth_ref import rows_for
    rng = np.random.default_rng(seed)
    lengths = [LONG] + [int(v) for v in rng.integers(0, 6, 40)] + [70]
    off = np.cumsum([0] + lengths).astype(np.int64)
    N = int(off[-1])
    x = np.concatenate([rows_for(200 + f, 1, J, C, score, seed=seed + 5) for f in range(N)])
    x[0, :, :C] = np.abs(x[0, :, :C])
    runs = ((60, 69), (128, 192), (192, 257), (0, 71), (LONG - 64, LONG))
    for i, (f0, f1) in enumerate(runs):
        j = i % J
        if f0 > 0:
            x[f0 - 1, j, :C], x[f0 - 1, j, C:] = 100.0 + i, 0.9      # a usable frame on either side, whatever rows_for put there
        if f1 < LONG:
            x[f1, j, :C], x[f1, j, C:] = 200.0 + i, 0.9
        gate(x, C, score, slice(f0, f1), j)
    gate(x, C, score, slice(int(off[-2]), N), 0)
    if offsets == "clamped":
        off[0], off[-1] = -5, N + 9
    elif offsets == "inner":
        off[0], off[-1] = 2, N - 3
    return x, off
