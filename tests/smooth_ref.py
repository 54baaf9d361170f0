"""Shared by tests/test_smooth_cpu.py, tests/test_smooth_host_cpu.py and tests/test_gpu_smooth.py (not a test): the One-Euro rule of include/kasf.h
(kasf_one_euro_push / _tracked / _tracks) in numpy, in fp32 -- one numpy operation per rounded operation of the rule, on numpy scalars of one type, never a
Python float -- and in fp64 (``ft=np.float64``: the same statements on the upcast inputs and parameters).

``push_np`` and ``tracked_np`` walk the joints one by one as the rule is written; ``step_arrays`` (under ``tracks_np`` and ``push_rows_np``) is a second
statement of the same rule over whole arrays with masks, so "a recorded track equals push frame by frame" compares two texts.  The row rule of the tracked entry is tests/tracked_ref.py's ``tracked_front_np``."""
import numpy as np

from tests.tracked_ref import tracked_front_np

TWO_PI = np.float32(6.2831855)
LIMIT = np.float32(1e12)


def params(rate=30.0, min_cutoff=1.0, beta=0.01, d_cutoff=1.0, min_score=0.3, max_hold=15):
    """The parameters as the entry points receive them: fp32, dt = 1 / rate rounded once."""
    return dict(dt=np.float32(1.0 / rate), min_cutoff=np.float32(min_cutoff), d_cutoff=np.float32(d_cutoff), beta=np.float32(beta),
                min_score=np.float32(min_score), max_hold=int(max_hold))


def new_state(S, J, C, ft=np.float32, fill=0.0):
    """xhat, dxhat [S,J,C] (any initial value: never read before written), last [S,J] all -1, owner [S] zeros; count [S] serves tracked_front_np only."""
    return dict(xhat=np.full((S, J, C), fill, ft), dxhat=np.full((S, J, C), fill, ft), last=np.full((S, J), -1, np.int64), owner=np.zeros(S, np.int32),
                count=np.zeros(S, np.int64), ring=np.zeros((S, 1, 1, 1), np.float32))


def _joint(p, ft, xj, C, has_score, tick, xhat, dxhat, last, restart):
    """One joint, steps 1-6 of the rule; xhat, dxhat [C] and last [()] are views into the state.  Returns the joint's output [Ct]."""
    out = xj.astype(ft)                                            # the score channel, and the input "as it came"
    m = [ft(xj[c]) for c in range(C)]
    usable = all(np.isfinite(v) and abs(v) <= ft(LIMIT) for v in m)
    if has_score:
        usable = usable and bool(xj[C] >= p["min_score"])          # False for a NaN score
    if restart:
        last[...] = -1
    k = max(int(tick) - int(last), 1)
    have = int(last) >= 0 and k - 1 <= p["max_hold"]
    if not have:
        if usable:
            xhat[:], dxhat[:], last[...] = m, ft(0), tick
        return out
    if not usable:
        out[:C] = xhat
        return out
    one, two_pi = ft(1), ft(TWO_PI)
    dt, min_cutoff, d_cutoff, beta = ft(p["dt"]), ft(p["min_cutoff"]), ft(p["d_cutoff"]), ft(p["beta"])
    dtj = ft(k) * dt
    rd = two_pi * d_cutoff
    rd = rd * dtj
    ad = rd + one
    ad = rd / ad
    for c in range(C):
        xh, dxh = xhat[c], dxhat[c]
        e = m[c] - xh
        d = e / dtj
        dx = d - dxh
        dx = ad * dx
        dx = dxh + dx
        fc = beta * abs(dx)
        fc = min_cutoff + fc
        r = two_pi * fc
        r = r * dtj
        a = r + one
        a = r / a
        xnew = a * e
        xnew = xh + xnew
        xhat[c], dxhat[c], out[c] = xnew, dx, xnew
    last[...] = tick
    return out


def _row(p, ft, x_row, has_score, tick, state, g, restart=False):
    J, C = state["last"].shape[1], state["xhat"].shape[2]
    with np.errstate(all="ignore"):
        return np.stack([_joint(p, ft, x_row[j], C, has_score, tick, state["xhat"][g, j], state["dxhat"][g, j], state["last"][g, j:j + 1].reshape(()), restart)
                         for j in range(J)])


def push_np(state, p, x, slots, tick, has_score, ft=np.float32):
    """kasf_one_euro_push: x [K,J,Ct] fp32, slots [K] or None, state updated in place -> out [K,J,Ct] of type ft.  An id outside [0, S) copies through."""
    S = state["last"].shape[0]
    out = np.empty(x.shape, ft)
    for i in range(x.shape[0]):
        g = i if slots is None else int(slots[i])
        out[i] = _row(p, ft, x[i], has_score, tick, state, g) if 0 <= g < S else x[i].astype(ft)
    return out


def tracked_np(state, p, x, track_arrays, rows, R, tick, has_score, ft=np.float32):
    """kasf_one_euro_tracked: x [B*R,J,Ct]; the rows resolved by tracked_front_np (which restarts owner / count) -> (out, row_slot, reset, why)."""
    row_slot, reset, why = tracked_front_np(state, track_arrays, rows, R)
    out = np.empty(x.shape, ft)
    for row in range(x.shape[0]):
        g = int(row_slot[row])
        out[row] = _row(p, ft, x[row], has_score, tick, state, g, restart=bool(reset[row])) if g >= 0 else x[row].astype(ft)
    return out, row_slot, reset, why


def step_arrays(p, x, has_score, tick, xhat, dxhat, last, ft=np.float32):
    """The rule once more, over whole arrays with masks: x [..., J, Ct]; xhat, dxhat [..., J, C] and last [..., J] are updated in place -> out [..., J, Ct]."""
    C = xhat.shape[-1]
    out = x.astype(ft)
    one, two_pi = ft(1), ft(TWO_PI)
    dt, min_cutoff, d_cutoff, beta = ft(p["dt"]), ft(p["min_cutoff"]), ft(p["d_cutoff"]), ft(p["beta"])
    m = out[..., :C].copy()
    with np.errstate(all="ignore"):
        usable = (np.isfinite(m) & (np.abs(m) <= ft(LIMIT))).all(-1)
        if has_score:
            usable &= x[..., C] >= p["min_score"]
        k = np.maximum(tick - last, 1)
        have = (last >= 0) & (k - 1 <= p["max_hold"])
        dtj = (k.astype(ft) * dt)[..., None]
        rd = two_pi * d_cutoff * dtj
        ad = rd / (rd + one)
        e = m - xhat
        dx = dxhat + ad * (e / dtj - dxhat)
        r = two_pi * (min_cutoff + beta * np.abs(dx)) * dtj
        xnew = xhat + r / (r + one) * e
    first, update, hold = ~have & usable, have & usable, have & ~usable
    out[..., :C][hold] = xhat[hold]
    out[..., :C][update] = xnew[update]
    xhat[first], dxhat[first] = m[first], 0
    xhat[update], dxhat[update] = xnew[update], dx[update]
    last[first | update] = tick
    return out


def push_rows_np(state, p, x, slots, tick, has_score, ft=np.float32):
    """push_np through step_arrays: every row of the call at once (slots: distinct ids in [0, S), or None)."""
    if slots is None:
        return step_arrays(p, x, has_score, tick, state["xhat"], state["dxhat"], state["last"], ft)
    xhat, dxhat, last = state["xhat"][slots], state["dxhat"][slots], state["last"][slots]
    out = step_arrays(p, x, has_score, tick, xhat, dxhat, last, ft)
    state["xhat"][slots], state["dxhat"][slots], state["last"][slots] = xhat, dxhat, last
    return out


def tracks_np(p, x, offsets, has_score, ft=np.float32):
    """kasf_one_euro_tracks: x [N,J,Ct] packed, offsets [P+1] -> out [N,J,Ct] of type ft, through step_arrays: every track from an empty state, tick = frame
    index."""
    N, J, Ct = x.shape
    C = Ct - (1 if has_score else 0)
    out = x.astype(ft)
    for t in range(len(offsets) - 1):
        xhat, dxhat, last = np.zeros((J, C), ft), np.zeros((J, C), ft), np.full(J, -1, np.int64)
        for tick, f in enumerate(range(int(offsets[t]), int(offsets[t + 1]))):
            out[f] = step_arrays(p, x[f], has_score, tick, xhat, dxhat, last, ft)
    return out


SHAPES = ((17, 2, True), (17, 3, False), (1, 1, False), (70, 2, True))       # (J, C, score): keypoints, poses, the smallest row, one that walks the lane loop


def rows_for(tick, n_rows, J, C, score, seed=0):
    """Rows [n_rows,J,C + score] cut from tracked_ref.frames_for's keypoints (pixel x, y in [0, 1000), confidence in [0, 1): min_score = 0.3 gates about 30 % of
    the joints), with a NaN and an infinity put in now and then, which is all that gates a row without a score."""
    from tests.tracked_ref import frames_for
    m = (J + 16) // 17
    x = np.ascontiguousarray(frames_for(tick, n_rows * m, seed).reshape(n_rows, m * 17, 3)[:, :J, [0, 1, 2][:C] + ([2] if score else [])])
    if tick % 5 == 3:
        x[0, 0, 0] = np.nan
    if tick % 7 == 4:
        x[-1, J - 1, C - 1] = np.inf
    if score and tick % 6 == 5:
        x[0, J - 1, C] = np.nan
    return x
