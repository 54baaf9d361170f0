"""The SORT tracker's rules (include/kasf.h, kasf_sort_update) without a GPU: a dense fp64 numpy restatement, ``sort_update_np``, held to the fixture the
reference's own ``Sort.update`` wrote (tests/golden/make_track_golden.py), the block structure of P the kernel relies on, the conditions under which the test
sequences have one answer, and every refusal that needs no device.  tests/test_gpu_track.py holds the kernel to ``sort_update_np`` on the sequences built here.

The filter arithmetic is this project's restatement of filterpy's ``KalmanFilter.predict`` / ``update`` (filterpy is not installed): the fixture pins the
reference's BOOKKEEPING -- association, threshold, births, deaths, output order, ids -- and its boxes through that restatement.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_sort.npz")
FRAME_W, FRAME_H = 1280.0, 720.0

# ---- the filter (sort.py:72-85) -------------------------------------------------------------------------------------------------------------------------
KF_F = np.eye(7)
KF_F[0, 4] = KF_F[1, 5] = KF_F[2, 6] = 1.0
KF_H = np.eye(4, 7)
KF_R = np.diag([1.0, 1.0, 10.0, 10.0])
KF_P0 = np.diag([10.0, 10.0, 10.0, 10.0, 1e4, 1e4, 1e4])
KF_Q = np.diag([1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.01 * 0.01])
BLOCK = np.zeros((7, 7), bool)                      # where P may be non-zero: (cx,vx), (cy,vy), (s,vs) and r
for _k in range(3):
    BLOCK[np.ix_([_k, _k + 4], [_k, _k + 4])] = True
BLOCK[3, 3] = True


def kf_predict_dense(x, P):
    return KF_F @ x, KF_F @ P @ KF_F.T + KF_Q


def kf_update_dense(x, P, z):
    """filterpy's KalmanFilter.update, restated from its published form."""
    y = z - KF_H @ x
    PHT = P @ KF_H.T
    S = KF_H @ PHT + KF_R
    K = PHT @ np.linalg.inv(S)
    x = x + K @ y
    I_KH = np.eye(7) - K @ KF_H
    return x, (I_KH @ P) @ I_KH.T + (K @ KF_R) @ K.T


def kf_predict_loop(x, P):
    """The same rules one scalar operation at a time (python floats: no BLAS, no fused multiply-add), with the products by the exact zeros and ones of F left
    out -- the sequence the kernel evaluates."""
    x, P = [float(v) for v in x], P.copy()
    x[0], x[1], x[2] = x[0] + x[4], x[1] + x[5], x[2] + x[6]
    for k in range(3):
        a, b, c, d = (float(P[k, k]), float(P[k, k + 4]), float(P[k + 4, k]), float(P[k + 4, k + 4]))
        fa, fb = a + c, b + d
        P[k, k], P[k, k + 4], P[k + 4, k], P[k + 4, k + 4] = (fa + fb) + 1.0, fb, c + d, d + float(KF_Q[k + 4, k + 4])
    P[3, 3] = float(P[3, 3]) + 1.0
    return np.array(x), P


def kf_update_loop(x, P, z):
    x, P = [float(v) for v in x], P.copy()
    for k in range(3):
        a, b, c, d = (float(P[k, k]), float(P[k, k + 4]), float(P[k + 4, k]), float(P[k + 4, k + 4]))
        r = float(KF_R[k, k])
        y = float(z[k]) - x[k]
        si = 1.0 / (a + r)
        kp, kv = a * si, c * si
        x[k], x[k + 4] = x[k] + kp * y, x[k + 4] + kv * y
        m, n = 1.0 - kp, 0.0 - kv
        ap0, ap1, ap2, ap3 = m * a, m * b, n * a + c, n * b + d
        P[k, k] = ap0 * m + (kp * r) * kp
        P[k, k + 4] = (ap0 * n + ap1) + (kp * r) * kv
        P[k + 4, k] = ap2 * m + (kv * r) * kp
        P[k + 4, k + 4] = (ap2 * n + ap3) + (kv * r) * kv
    a = float(P[3, 3])
    y = float(z[3]) - x[3]
    si = 1.0 / (a + 10.0)
    kk = a * si
    m = 1.0 - kk
    x[3] = x[3] + kk * y
    P[3, 3] = (m * a) * m + (kk * 10.0) * kk
    return np.array(x), P


KALMAN = {"dense": (kf_predict_dense, kf_update_dense), "loop": (kf_predict_loop, kf_update_loop)}


def box_to_z(b):
    w, h = b[2] - b[0], b[3] - b[1]
    return np.array([b[0] + w / 2.0, b[1] + h / 2.0, w * h, w / h])


def x_to_box(x):
    with np.errstate(all="ignore"):
        w = np.sqrt(x[2] * x[3])
        h = x[2] / w
        return np.array([x[0] - w / 2.0, x[1] - h / 2.0, x[0] + w / 2.0, x[1] + h / 2.0])


def iou_matrix(dets, trks):
    """sort.py:16-30 for every (detection, track) pair in fp64, rounded to fp32; a value that is not finite counts as 0."""
    d, t = dets[:, None, :], trks[None, :, :]
    with np.errstate(all="ignore"):
        w = np.maximum(0.0, np.minimum(d[..., 2], t[..., 2]) - np.maximum(d[..., 0], t[..., 0]))
        h = np.maximum(0.0, np.minimum(d[..., 3], t[..., 3]) - np.maximum(d[..., 1], t[..., 1]))
        wh = w * h
        o = wh / ((d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1]) + (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1]) - wh)
    o = np.where(np.isfinite(o), o, 0.0)
    return o.astype(F32)


def new_tracker(slots=32, max_age=1, min_hits=3, iou_threshold=0.3, num_person=1, hold_last=False):
    """An empty tracker of one stream: what an all-zero state buffer is."""
    return dict(slots=slots, max_age=max_age, min_hits=min_hits, iou_threshold=iou_threshold, num_person=num_person, hold_last=hold_last,
                tracks=[], next_id=0, ticks=0, held=None)


def sort_update_np(trk, dets, count=None, kalman="dense", iou_noise=None, probe=None):
    """One tick of include/kasf.h's rules on ``trk`` (``new_tracker``), dense fp64 numpy with ``np.linalg.inv``, ``@`` and scipy's assignment.
    ``dets`` [n,>=4] float32.  Returns a dict of what ``TrackResult`` holds for one stream (``boxes`` / ``persons`` in fp64, only the rows that count).
    ``iou_noise`` (a Generator -> uniform +-1e-6 on the IoU matrix the assignment sees) and ``probe`` (a list that receives per-tick diagnostics) serve the
    input-condition tests."""
    predict, update = KALMAN[kalman]
    dets = np.asarray(dets)
    assert dets.dtype == F32
    n = dets.shape[0] if count is None else max(0, min(int(count), dets.shape[0]))
    d = dets[:n, :4]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d).all(axis=1) & ((d[:, 3].astype(F64) - d[:, 1].astype(F64)) > 0)
    d = d[ok].astype(F64)
    if trk["hold_last"]:
        if len(d):
            trk["held"] = d.copy()
        elif trk["held"] is not None:
            d = trk["held"].copy()
    trk["ticks"] += 1
    # 1 predict; a non-finite box leaves
    kept = []
    for t in trk["tracks"]:
        if t["x"][6] + t["x"][2] <= 0:
            t["x"][6] *= 0.0
        t["x"], t["P"] = predict(t["x"], t["P"])
        t["age"] += 1
        if t["tsu"] > 0:
            t["streak"] = 0
        t["tsu"] += 1
        t["pred"] = x_to_box(t["x"])
        if np.isfinite(t["pred"]).all():
            kept.append(t)
    tracks = trk["tracks"] = kept
    nt, nd = len(tracks), len(d)
    # 2-4 association
    det_track = np.full(nd, -1)
    low = np.zeros(nd, bool)
    if nt and nd:
        iou = iou_matrix(d, np.stack([t["pred"] for t in tracks]))
        seen = iou.astype(F64) if iou_noise is None else iou.astype(F64) + iou_noise.uniform(-1e-6, 1e-6, iou.shape)
        rows, cols = linear_sum_assignment(-seen)
        for r, c in zip(rows, cols):
            det_track[r] = c
            low[r] = iou[r, c] < F32(trk["iou_threshold"])
        if probe is not None:
            probe.append(dict(iou=iou, rows=rows, cols=cols))
    # 5 update
    for di in range(nd):
        if det_track[di] >= 0 and not low[di]:
            t = tracks[det_track[di]]
            t["tsu"], t["hits"], t["streak"] = 0, t["hits"] + 1, t["streak"] + 1
            t["x"], t["P"] = update(t["x"], t["P"], box_to_z(d[di]))
    # 6 births
    order = [di for di in range(nd) if det_track[di] < 0] + [di for di in range(nd) if det_track[di] >= 0 and low[di]]
    n_before, dropped = nt, 0
    for di in order:
        if len(tracks) >= trk["slots"]:
            dropped += 1
            continue
        used = {t["slot"] for t in tracks}
        slot = min(s for s in range(trk["slots"]) if s not in used)
        x = np.zeros(7)
        x[:4] = box_to_z(d[di])
        tracks.append(dict(x=x, P=KF_P0.copy(), id=trk["next_id"], slot=slot, tsu=0, hits=0, streak=0, age=0, pred=None))
        trk["next_id"] += 1
    # 7 emit newest first, then deaths
    rows = []
    for p in range(len(tracks) - 1, -1, -1):
        t = tracks[p]
        if t["tsu"] < 1 and (t["streak"] >= trk["min_hits"] or trk["ticks"] <= trk["min_hits"]):
            rows.append((x_to_box(t["x"]), t["id"] + 1, t["slot"], int(p >= n_before)))
    trk["tracks"] = [t for t in tracks if not t["tsu"] > trk["max_age"]]
    boxes = np.array([r[0] for r in rows], F64).reshape(-1, 4)
    pc = min(len(rows), trk["num_person"])
    return dict(boxes=boxes, ids=np.array([r[1] for r in rows], np.int32), slot=np.array([r[2] for r in rows], np.int32),
                born=np.array([r[3] for r in rows], np.int32), count=len(rows), dropped=dropped, persons=boxes[::-1][:pc].copy(), person_count=pc)


def tracker_state_np(trk):
    """What ``SortTracker.state()`` shows for one stream: x, P, box and the counters per list position."""
    ts = trk["tracks"]
    ints = {k: np.array([t[k] for t in ts], np.int32) for k in ("id", "slot", "tsu", "hits", "streak", "age")}
    return dict(x=np.array([t["x"] for t in ts], F64).reshape(-1, 7), P=np.array([t["P"] for t in ts], F64).reshape(-1, 7, 7),
                boxes=np.array([x_to_box(t["x"]) for t in ts], F64).reshape(-1, 4), tracks=len(ts), next_id=trk["next_id"], ticks=trk["ticks"], **ints)


# ---- the sequences (shared with tests/test_gpu_track.py and the fixture generator) ---------------------------------------------------------------------
def players(seed, people, ticks=40, p_miss=0.05, p_fp=0.04, absent=None, grid=None, box=((40, 70), (100, 160)), speed=3.0, noise=1.0):
    """Seeded synthetic players in a 1280 x 720 frame: constant velocity plus corner noise, detection order shuffled every tick, random misses and false
    positives -> a list of ``ticks`` float32 arrays [n_t, 5] (x1, y1, x2, y2, score).  ``absent``: {person: [(first, last), ...]} ticks without that person.
    ``grid``: (columns, rows) of cells the players start in (default: one row)."""
    g = np.random.default_rng(seed)
    cols, rows = grid or (people, 1)
    cw, ch = FRAME_W / cols, FRAME_H / rows
    w, h = g.uniform(*box[0], people), g.uniform(*box[1], people)
    cx = (np.arange(people) % cols + 0.5) * cw + g.uniform(-0.1, 0.1, people) * cw
    cy = (np.arange(people) // cols + 0.5) * ch + g.uniform(-0.1, 0.1, people) * ch
    vx, vy = g.uniform(-speed, speed, people), g.uniform(-speed / 3, speed / 3, people)
    seq = []
    for t in range(ticks):
        out = []
        for p in range(people):
            gone = any(a <= t <= b for a, b in (absent or {}).get(p, ()))
            miss = g.uniform() < p_miss                              # drawn whether or not the player is there: one stream of random numbers per seed
            e = g.normal(0.0, noise, 4)
            if gone or miss:
                continue
            x, y = cx[p] + vx[p] * t, cy[p] + vy[p] * t
            out.append([x - w[p] / 2 + e[0], y - h[p] / 2 + e[1], x + w[p] / 2 + e[2], y + h[p] / 2 + e[3], g.uniform(0.7, 1.0)])
        if g.uniform() < p_fp:
            fx, fy = g.uniform(0, FRAME_W - 80), g.uniform(0, FRAME_H - 150)
            out.append([fx, fy, fx + g.uniform(30, 80), fy + g.uniform(60, 150), g.uniform(0.3, 0.7)])
        out = np.array(out, F64).reshape(-1, 5)
        seq.append(out[g.permutation(len(out))].astype(F32))
    return seq


def greedy_sequence():
    """Two ticks.  Tick 0 founds three tracks; on tick 1 detection 0 overlaps tracks 0 (0.85) and 1 (0.79), detection 1 overlaps track 0 (0.6) and track 1
    (0.38): best-IoU-first matching takes (0,0) and is left with (1,1) = 1.23 in all, the optimum is (0,1) + (1,0) = 1.39."""
    t0 = np.array([[0, 0, 100, 200, 1], [20, 0, 120, 200, 1], [600, 300, 660, 420, 1]], F32)
    t1 = np.array([[8, 0, 108, 200, 1], [-25, 0, 75, 200, 1], [601, 301, 661, 421, 1]], F32)
    return [t0, t1, t1.copy()]


def with_bad_rows(seq, seed):
    """The same sequence with rows that must be ignored pushed in front of, between and behind the real ones: NaN, +-inf, h = 0, h < 0."""
    g = np.random.default_rng(seed)
    bad = np.array([[np.nan, 5, 50, 90, 1], [10, 20, np.inf, 90, 1], [10, -np.inf, 50, 90, 1], [100, 300, 160, 300, 1], [100, 300, 160, 250, 1]], F32)
    out = []
    for t, d in enumerate(seq):
        if t % 3 == 1:
            k = g.integers(0, len(bad))
            at = g.integers(0, len(d) + 1)
            d = np.concatenate((d[:at], bad[k:k + 1], d[at:]))
        out.append(d)
    return out


def pad(seq, rows):
    """-> dets [T, rows, 5] float32 (rows past a tick's count hold a box that would match everything, to show the count is respected) and count [T] int32."""
    dets = np.empty((len(seq), rows, 5), F32)
    dets[...] = np.array([0, 0, FRAME_W, FRAME_H, 1], F32)
    count = np.zeros(len(seq), np.int32)
    for t, d in enumerate(seq):
        assert len(d) <= rows
        dets[t, :len(d)], count[t] = d, len(d)
    return dets, count


def empty_ticks(seq, ticks):
    return [d[:0] if t in ticks else d for t, d in enumerate(seq)]


# name -> (tracker parameters, sequence, rows of the padded detections).  Seeds were chosen so that every sequence meets the two input conditions below
# (test_sequences_have_one_answer): a seed that does not is replaced, never excused.
def build_cases():
    c = {}
    c["overflow"] = (dict(slots=3, min_hits=0), players(11, 5, absent={1: [(12, 40)]}), 8)                      # 5 people, 3 slots: births dropped and counted
    c["full64"] = (dict(slots=64, min_hits=0), players(12, 64, grid=(8, 8), box=((30, 50), (40, 60)), speed=1.0, p_miss=0.0, p_fp=0.0), 64)
    c["demo"] = (dict(slots=32, min_hits=0, num_person=3), players(13, 2, absent={1: [(0, 9)]}), 6)            # fewer emitted than num_person, then a late entry
    c["default"] = (dict(slots=32, min_hits=3, num_person=1), players(14, 5, absent={3: [(0, 14)], 0: [(25, 40)]}), 8)
    c["max_age2"] = (dict(slots=8, min_hits=0, max_age=2), players(15, 3, p_miss=0.0, absent={1: [(10, 11)], 2: [(20, 40)]}), 6)   # a two-tick miss, re-matched
    c["birth_death"] = (dict(slots=8, min_hits=0), players(16, 3, p_miss=0.0, p_fp=0.0, absent={0: [(10, 40)], 2: [(0, 10)]}), 6)  # track 0 dies on tick 11, where 2 is born
    c["bad_rows"] = (dict(slots=8, min_hits=3), with_bad_rows(players(17, 4), 5), 8)
    c["hold_on"] = (dict(slots=8, min_hits=0, hold_last=True), empty_ticks(players(18, 3, p_fp=0.0), {0, 1, 7, 8, 20}), 6)
    c["hold_off"] = (dict(slots=8, min_hits=0, hold_last=False), empty_ticks(players(18, 3, p_fp=0.0), {0, 1, 7, 8, 20}), 6)
    c["greedy"] = (dict(slots=4, min_hits=0), greedy_sequence(), 3)
    return c


CASES = build_cases()


def run_np(params, seq, kalman="dense", iou_noise=None, probe=None, states=False):
    trk = new_tracker(**params)
    out = []
    for d in seq:
        r = sort_update_np(trk, d, kalman=kalman, iou_noise=iou_noise, probe=probe)
        if states:
            r["state"] = tracker_state_np(trk)
        out.append(r)
    return out


DISCRETE = ("ids", "slot", "born", "count", "dropped", "person_count")


def same_discrete(a, b):
    return all(np.array_equal(ra[k], rb[k]) for ra, rb in zip(a, b) for k in DISCRETE)


def fixture():
    return np.load(GOLDEN, allow_pickle=False)


FIXTURE_CASES = ("demo", "default", "max_age2", "birth_death", "greedy", "full64")       # what the reference can run: no cap, no bad rows, no hold


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_loads_without_pickles_and_is_small():
    assert os.path.getsize(GOLDEN) < 1 << 20
    z = fixture()
    for name in FIXTURE_CASES:
        dets, count = pad(CASES[name][1], CASES[name][2])
        assert np.array_equal(z[f"{name}_dets"], dets) and np.array_equal(z[f"{name}_count"], count), f"{name}: the fixture was written for other detections"


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_restatement_reproduces_the_reference_tick_by_tick(name):
    z = fixture()
    params, seq, _ = CASES[name]
    got = run_np(params, seq)
    ret, ret_n = z[f"{name}_ret"], z[f"{name}_ret_count"]
    assert len(got) == len(ret_n)
    worst = 0.0
    for t, r in enumerate(got):
        want = ret[t, :ret_n[t]]
        assert r["count"] == ret_n[t], (name, t)
        assert np.array_equal(r["ids"], want[:, 4].astype(np.int32)), (name, t)            # ids and row order
        if r["count"]:
            worst = max(worst, float(np.abs(r["boxes"] - want[:, :4]).max()))
    assert worst <= 1e-9 * FRAME_W, worst                                                   # fp64 round-off of two restatements of the same filter


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_P_keeps_its_blocks_exactly(name):
    params, seq, _ = CASES[name]
    n = 0
    for r in run_np(params, seq, states=True):
        P = r["state"]["P"]
        assert np.isfinite(P).all()
        assert (P[:, ~BLOCK] == 0).all(), name
        n += len(P)
    assert n > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_sequences_have_one_answer(name):
    """The conditions under which a kernel and scipy must agree: no matched pair within 1e-4 of the threshold, and no discrete output that moves when the
    IoU matrix the assignment sees is perturbed by +-1e-6."""
    params, seq, _ = CASES[name]
    probe = []
    base = run_np(params, seq, probe=probe)
    assert probe
    for p in probe:
        m = p["iou"][p["rows"], p["cols"]].astype(F64)
        assert (np.abs(m - 0.3) >= 1e-4).all(), name
    for seed in (1, 2, 3):
        assert same_discrete(base, run_np(params, seq, iou_noise=np.random.default_rng(seed))), (name, seed)


def test_cases_reach_what_they_are_for():
    res = {k: run_np(v[0], v[1], states=True) for k, v in CASES.items()}
    assert max(r["dropped"] for r in res["overflow"]) >= 2 and max(r["state"]["tracks"] for r in res["overflow"]) == 3
    assert any(r["born"].any() for r in res["overflow"][5:]), "a freed slot is taken again"
    assert all(r["count"] == 64 and r["state"]["tracks"] == 64 for r in res["full64"])
    assert any(0 < r["count"] < 3 and r["person_count"] == r["count"] for r in res["demo"]) and any(r["person_count"] == 3 for r in res["demo"])
    assert res["default"][0]["count"] > 0, "ticks <= min_hits: emitted from the first tick"
    assert any(int((r["state"]["tsu"] == 0).sum()) > r["count"] for r in res["default"][4:]), "min_hits = 3 holds a matched young track back"
    st = [r["state"] for r in res["max_age2"]]
    assert any(s["tsu"].max(initial=0) == 2 for s in st) and st[12]["tracks"] == 3 and (st[12]["tsu"] == 0).all(), "two ticks missed, then matched again"
    bd = [r["state"] for r in res["birth_death"]]
    assert any(r["born"].any() and now["tracks"] == before["tracks"] and now["next_id"] == before["next_id"] + 1
               for before, now, r in zip(bd[5:], bd[6:], res["birth_death"][6:])), "a birth and a death on one tick"
    on, off = res["hold_on"], res["hold_off"]
    assert on[0]["count"] == 0 and on[7]["count"] > 0 and off[7]["count"] == 0
    more = [len(d) for d in CASES["default"][1]]
    trk = [r["state"]["tracks"] for r in res["default"]]
    assert any(m > n for m, n in zip(more[1:], trk[:-1])) and any(0 < m < n for m, n in zip(more[1:], trk[:-1])), "more detections than tracks, and the reverse"
    # the greedy tick: best-IoU-first gives another matching than the optimum
    probe = []
    run_np(*CASES["greedy"][:2], probe=probe)
    iou = probe[0]["iou"].astype(F64).copy()
    optimum = sorted(zip(probe[0]["rows"].tolist(), probe[0]["cols"].tolist()))
    greedy = []
    while (iou > 0).any():
        r, c = np.unravel_index(np.argmax(iou), iou.shape)
        greedy.append((int(r), int(c)))
        iou[r, :], iou[:, c] = -1, -1
    assert sorted(greedy) != optimum and len(greedy) == 3


def loop_vs_dense():
    """Largest difference between the dense BLAS / LAPACK evaluation and the explicit-loop evaluation of the same rules over every case: x and boxes relative
    to the frame width, P relative to max |P|."""
    worst_x = worst_p = 0.0
    for name, (params, seq, _) in CASES.items():
        a, b = run_np(params, seq, states=True), run_np(params, seq, kalman="loop", states=True)
        assert same_discrete(a, b), name
        for ra, rb in zip(a, b):
            sa, sb = ra["state"], rb["state"]
            if len(sa["x"]):
                xs = np.array([FRAME_W, FRAME_W, FRAME_W * FRAME_W, 1.0, FRAME_W, FRAME_W, FRAME_W * FRAME_W])
                worst_x = max(worst_x, float((np.abs(sa["x"] - sb["x"]) / xs).max()), float(np.abs(sa["boxes"] - sb["boxes"]).max() / FRAME_W))
                worst_p = max(worst_p, float(np.abs(sa["P"] - sb["P"]).max() / np.abs(sa["P"]).max()))
    return worst_x, worst_p


# Measured where this was written (numpy 2.2.6, 40 ticks of every case): 0.0 and 0.0 -- numpy's 7 x 7 products and LAPACK's inverse of the diagonal S
# round exactly as the explicit loop does, so the two forms are bit-equal.  tests/test_gpu_track.py allows the kernel 64 x these against the dense form with
# a floor of 1e-12: the floor is the tolerance (1.3e-9 pixels on x and the boxes).
LOOP_VS_DENSE_X = 0.0
LOOP_VS_DENSE_P = 0.0


def test_loop_form_is_the_dense_form_up_to_rounding():
    wx, wp = loop_vs_dense()
    print(f"loop vs dense: x / boxes {wx:.3e} of the frame width, P {wp:.3e} of max |P|")
    assert wx <= max(LOOP_VS_DENSE_X, 1e-12 / 64) and wp <= max(LOOP_VS_DENSE_P, 1e-12 / 64), (wx, wp)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def entry_args():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    nbytes = lib.kasf_sort_state_bytes(1, 4, 8)
    bufs = dict(state=np.full(nbytes, 3, np.uint8), dets=np.full(8 * 5, 5, F32), cnt=np.full(1, 2, np.int32), boxes=np.full(16, 7, F32),
                ids=np.full(4, 9, np.int32), slot=np.full(4, 9, np.int32), born=np.full(4, 9, np.int32), count=np.full(1, 9, np.int32),
                dropped=np.full(1, 9, np.int32), persons=np.full(4, 7, F32), pc=np.full(1, 9, np.int32))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(state="state", streams=1, slots=4, max_dets=8, dets="dets", det_rows=8, sstride=40, rstride=5, cnt="cnt", max_age=1, min_hits=3, thr=0.3,
             num_person=1, hold=0, boxes="boxes", ids="ids", slot="slot", born="born", count="count", dropped="dropped", persons="persons", pc="pc"):
        p = lambda k: None if k is None else vp(bufs[k])
        return lib.kasf_sort_update(p(state), streams, slots, max_dets, p(dets), det_rows, sstride, rstride, p(cnt), max_age, min_hits, thr, num_person, hold,
                                    p(boxes), p(ids), p(slot), p(born), p(count), p(dropped), p(persons), p(pc), None)

    return call, bufs


REFUSED = [dict(streams=-1), dict(streams=65536), dict(slots=0), dict(slots=65), dict(slots=-1), dict(max_dets=0), dict(max_dets=65), dict(det_rows=-1),
           dict(det_rows=9), dict(rstride=3), dict(rstride=0), dict(sstride=-1), dict(max_age=-1), dict(min_hits=-1), dict(thr=float("nan")),
           dict(thr=float("inf")), dict(num_person=0), dict(num_person=65536), dict(state=None), dict(dets=None), dict(boxes=None), dict(ids=None),
           dict(slot=None), dict(born=None), dict(count=None), dict(dropped=None), dict(persons=None), dict(pc=None)]


def test_entry_points_refuse_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    assert {"kasf_sort_update", "kasf_sort_state_bytes"} <= set(_lib.SIGNATURES)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, os.pardir, "include", "kasf.h")).read()
    assert "int kasf_sort_update(void* state, int32_t streams, int32_t slots, int32_t max_dets, const float* dets, int32_t det_rows," in hdr
    assert "RESTATED from the published form of filterpy's KalmanFilter.update" in hdr and "ALL ZERO IS AN EMPTY TRACKER" in hdr
    assert _lib.ABI_VERSION == lib.kasf_version() == 12
    assert lib.kasf_sort_state_bytes(1, 4, 8) == 64 + 4 * 184 + 8 * 16 and lib.kasf_sort_state_bytes(3, 64, 64) == 3 * (64 + 64 * 184 + 64 * 16)
    assert lib.kasf_sort_state_bytes(0, 1, 1) == 0
    for bad in ((-1, 4, 8), (65536, 4, 8), (1, 0, 8), (1, 65, 8), (1, 4, 0), (1, 4, 65)):
        assert lib.kasf_sort_state_bytes(*bad) == -2 and lib.kasf_last_error(), bad
    call, bufs = entry_args()
    keep = {k: v.copy() for k, v in bufs.items()}
    assert call(streams=0) == 0 and call(streams=0, state=None, dets=None, boxes=None) == 0          # nothing to do
    for kw in REFUSED:
        assert call(**kw) == 2, kw
        assert lib.kasf_last_error(), kw
    assert all(np.array_equal(bufs[k], keep[k]) for k in bufs), "a refused call touches no buffer"


def test_python_surface_refuses_before_any_launch():
    import kasportsformer_amd as K
    assert {"SortTracker", "TrackResult"} <= set(K.__all__) and "SortTracker" in K.__doc__
    assert "min_hits=0" in K.SortTracker.__doc__
    from kasportsformer_amd import track
    import inspect
    sig = inspect.signature(K.SortTracker.__init__).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [("streams", 1), ("slots", 32), ("max_age", 1), ("min_hits", 3), ("iou_threshold", 0.3),
                                                            ("num_person", 1), ("hold_last", False), ("device", None)]
    with pytest.raises(RuntimeError):
        K.SortTracker(device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            K.SortTracker()
    for exc, kw in ((ValueError, dict(streams=0)), (ValueError, dict(streams=65536)), (ValueError, dict(slots=0)), (ValueError, dict(slots=65)),
                    (ValueError, dict(max_age=-1)), (ValueError, dict(min_hits=-1)), (ValueError, dict(num_person=0)), (ValueError, dict(iou_threshold=float("nan"))),
                    (TypeError, dict(slots=3.5)), (TypeError, dict(streams="2")), (TypeError, dict(min_hits=True)), (TypeError, dict(iou_threshold="x"))):
        with pytest.raises(exc):
            K.SortTracker(**kw)
    b = np.zeros((2, 5, 6), F32)
    chk = track.check_update_args
    t, c = chk(b, None, 2)
    assert tuple(t.shape) == (2, 5, 6) and c is None
    t, c = chk(b[0], [3], 1)
    assert tuple(t.shape) == (1, 5, 6) and c.dtype == torch.int32 and c.tolist() == [3]
    for exc, call in ((TypeError, lambda: chk(b.astype(F64), None, 2)),
                      (TypeError, lambda: chk(b.tolist(), None, 2)),
                      (TypeError, lambda: chk(b, np.zeros(2, F32), 2)),
                      (ValueError, lambda: chk(b[:, :, :3], None, 2)),
                      (ValueError, lambda: chk(b[0, 0], None, 1)),
                      (ValueError, lambda: chk(b, None, 3)),
                      (ValueError, lambda: chk(np.zeros((1, 65, 4), F32), None, 1)),
                      (ValueError, lambda: chk(b, [1, 6], 2)),
                      (ValueError, lambda: chk(b, [-1, 2], 2)),
                      (ValueError, lambda: chk(b, [1, 2, 3], 2))):
        with pytest.raises(exc):
            call()
