"""Host side of the One-Euro filter (kasportsformer_amd.OneEuroFilter / smooth_tracks, kasf_one_euro_*): properties of the rule on its numpy restatement
(tests/smooth_ref.py), the restatement in fp32 against fp64, the refusals of the Python surface and of the three entry points without a device, the header,
the Makefile and the command line."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.smooth_ref import SHAPES, new_state, params, push_np, rows_for, tracked_np, tracks_np
from tests.tracked_ref import Cases, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max |fp32 restatement - fp64 restatement| measured on fp32_inputs() below (pixels; coordinates up to about 1,000 px, 300 ticks, 30 % of the joints gated):
# deterministic on one numpy build, the factor 4 is for others.  It is 1.4 ulps of a coordinate near 1,000 (6.1e-5 each), 8.7e-8 relative.
FP32_MEASURED = 8.55e-5
FP32_BAR = 4 * FP32_MEASURED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def one_slot(xs, p, score, ft=np.float32, ticks=None):
    """xs [n,J,Ct] pushed to one slot tick by tick -> ([n,J,Ct] outputs, the state)."""
    st = new_state(1, xs.shape[1], xs.shape[2] - int(score), ft)
    out = [push_np(st, p, xs[i:i + 1], None, i if ticks is None else ticks[i], score, ft)[0] for i in range(len(xs))]
    return np.stack(out), st


# ---- properties of the rule ----
def test_constant_input_comes_back_bit_for_bit():
    g = np.random.default_rng(5)
    row = np.zeros((20, 3), np.float32)
    row[:, :2] = (g.random((20, 2)) * 2000.0).astype(np.float32)                      # 40 random coordinates in [0, 2000)
    row[:, 2] = 0.9
    row[0, :2] = [0.0, 1999.9999]
    for p in (params(), params(beta=5.0, min_cutoff=0.05, d_cutoff=3.0), params(rate=1000.0)):
        out, _ = one_slot(np.repeat(row[None], 60, 0), p, True)
        assert np.array_equal(bits(out), bits(np.repeat(row[None], 60, 0)))
    assert np.array_equal(bits(tracks_np(params(), np.repeat(row[None], 60, 0), [0, 60], True)), bits(np.repeat(row[None], 60, 0)))


def test_first_sample_is_passed_through():
    for J, Cn, score in SHAPES:
        x = rows_for(1, 3, J, Cn, score)
        st = new_state(3, J, Cn, fill=-7.0)
        out = push_np(st, params(), x, None, 0, score)
        assert np.array_equal(bits(out), bits(x))
        usable = np.isfinite(x[..., :Cn]).all(-1) & ((x[..., Cn] >= np.float32(0.3)) if score else True)
        assert np.array_equal(st["last"] == 0, usable) and np.array_equal(st["last"] == -1, ~usable)
        assert np.array_equal(st["xhat"][usable], x[..., :Cn][usable]) and not st["dxhat"][usable].any() and (st["xhat"][~usable] == -7.0).all()


def test_beta_zero_is_the_exponential_filter():
    g = np.random.default_rng(6)
    n = 200
    x = np.zeros((n, 4, 2), np.float32)
    x[:] = (500.0 + 300.0 * np.sin(np.arange(n)[:, None, None] / 9.0 + g.random((1, 4, 2)) * 6.0) + g.normal(0.0, 2.0, (n, 4, 2))).astype(np.float32)
    p = params(beta=0.0, min_cutoff=1.5)
    out, _ = one_slot(x, p, False)
    r = np.float64(np.float32(6.2831855)) * np.float64(p["min_cutoff"]) * np.float64(p["dt"])
    a = r / (r + 1.0)
    want = np.empty((n, 4, 2), np.float64)
    for i in range(n):                                             # xhat_i = (1 - a)^i x_0 + a sum_{q=1..i} (1 - a)^(i - q) x_q
        w = a * (1.0 - a) ** (i - np.arange(1, i + 1))
        want[i] = (1.0 - a) ** i * x[0] + np.tensordot(w, x[1:i + 1].astype(np.float64), 1)
    err = np.abs(out - want).max()
    print(f"beta = 0 against the closed form: {err:.3g} px (bar {FP32_BAR:.3g})")
    assert err <= FP32_BAR


def test_low_score_and_nan_joints_hold():
    p = params(min_score=0.3, max_hold=15)
    x = np.zeros((6, 3, 3), np.float32)
    x[:, :, :2] = np.arange(6, dtype=np.float32)[:, None, None] * 10.0 + 100.0
    x[:, :, 2] = 0.9
    x[2:5, 0, 2] = [0.29999, 0.05, np.nan]                         # joint 0: a low score, a lower one, a NaN score
    x[2, 1, 0], x[3, 1, 1], x[4, 1, 0] = np.nan, np.inf, -2e12     # joint 1: a NaN, an infinity, a value beyond 1e12; joint 2 is never gated
    out, st = one_slot(x, p, True)
    for j in (0, 1):
        assert np.array_equal(bits(out[2:5, j, :2]), bits(np.repeat(out[1:2, j, :2], 3, 0))), j       # held at the estimate after tick 1
        assert not np.array_equal(out[5, j, :2], out[1, j, :2]) and st["last"][0, j] == 5
    assert np.array_equal(bits(out[..., 2]), bits(x[..., 2]))                                       # the score is copied through, NaN included
    ref, _ = one_slot(x[:, 2:3], p, True)
    assert np.array_equal(bits(out[:, 2:3]), bits(ref))                                             # a joint does not see its neighbours' gates
    k3, _ = one_slot(x[[0, 1, 5], :1], p, True, ticks=[0, 1, 5])                                   # joint 0 with the gated ticks simply absent: k = 4
    assert np.array_equal(bits(out[5, :1]), bits(k3[2]))


@pytest.mark.parametrize("max_hold", [0, 1, 4])
def test_estimate_is_dropped_after_exactly_max_hold_missed_ticks(max_hold):
    p = params(min_score=0.3, max_hold=max_hold)

    def run(missed, last_usable):
        n = 2 + missed + 1
        x = np.zeros((n, 1, 3), np.float32)
        x[:, 0, :2] = 50.0 + 7.0 * np.arange(n, dtype=np.float32)[:, None]
        x[:, 0, 2] = 0.9
        x[2:2 + missed, 0, 2] = 0.1
        if not last_usable:
            x[-1, 0, 2] = 0.1
        return x, one_slot(x, p, True)[0]
    # a usable sample after `missed` gated ticks: filtered (not the input) up to max_hold of them, passed through as a first sample after one more
    x, out = run(max_hold, True)
    assert not np.array_equal(out[-1, 0, :2], x[-1, 0, :2])
    assert np.array_equal(bits(out[2:-1, 0, :2]), bits(np.repeat(out[1:2, 0, :2], max_hold, 0)))
    x, out = run(max_hold + 1, True)
    assert np.array_equal(bits(out[-1]), bits(x[-1]))
    # a gated sample: held through missed tick number max_hold + 1 (k - 1 = max_hold), the input as it came from the next one on
    x, out = run(max_hold, False)
    assert np.array_equal(bits(out[-1, 0, :2]), bits(out[1, 0, :2]))
    x, out = run(max_hold + 1, False)
    assert np.array_equal(bits(out[-1]), bits(x[-1])) and np.array_equal(bits(out[-2, 0, :2]), bits(out[1, 0, :2]))


@pytest.mark.parametrize("rows,R", [("persons", 2), ("tracks", 4)])
def test_restart_on_born_and_owner_change_follows_the_script(rows, R):
    """The tracked restatement against a second statement that keeps one single-slot filter per player."""
    B, S_t, T, J, Cn, score = 2, 4, 5, 17, 2, True
    p = params(min_score=0.3, max_hold=2)
    state, cases, players, holder = new_state(B * S_t, J, Cn, fill=-7.0), Cases(T, S_t, R), {}, {}
    seen = dict(hold=0, drop=0, update=0, first=0)
    for tick, arrays in enumerate(script(T, 3 * T + 4)):
        x = rows_for(tick, B * R, J, Cn, score, seed=T)
        owner_before, last_before = state["owner"].copy(), state["last"].copy()
        out, row_slot, reset, why = tracked_np(state, p, x, arrays, rows, R, tick, score)
        cases.see(tick, arrays, owner_before, state["owner"], state["count"], row_slot, reset, why)
        for row in range(B * R):
            b, k = divmod(row, R)
            if why[row] != "ok":
                assert row_slot[row] == -1 and np.array_equal(bits(out[row]), bits(x[row]))
                continue
            cb = min(max(int(arrays["count"][b]), 0), S_t)
            r = cb - 1 - k if rows == "persons" else k
            i, s, bn = int(arrays["ids"][b, r]), int(arrays["slot"][b, r]), int(arrays["born"][b, r])
            fresh = holder.get((b, s)) != i or bn != 0
            if fresh:
                players[(b, i)], holder[(b, s)] = new_state(1, J, Cn), i
            assert bool(reset[row]) == fresh, (tick, row)
            want = push_np(players[(b, i)], p, x[row:row + 1], None, tick, score)[0]
            assert np.array_equal(bits(out[row]), bits(want)), (tick, row)
            g = b * S_t + s
            assert np.array_equal(state["last"][g], players[(b, i)]["last"][0])
            usable = np.isfinite(x[row, :, :Cn]).all(-1) & (x[row, :, Cn] >= p["min_score"])
            lb = np.where(reset[row], -1, last_before[g])
            have = (lb >= 0) & (tick - lb - 1 <= p["max_hold"])
            seen["hold"] += int((have & ~usable).sum())
            seen["update"] += int((have & usable).sum())
            seen["first"] += int((~have & usable).sum())
            seen["drop"] += int(((lb >= 0) & ~have).sum())
    assert not cases.missing(), cases.missing()
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("J,Cn,score", SHAPES)
def test_smooth_tracks_equals_push_tick_by_tick(J, Cn, score):
    p = params(min_score=0.3, max_hold=2)
    lengths = [0, 1, 2, 40]
    off = np.cumsum([0] + lengths)
    x = np.concatenate([rows_for(100 + f, 1, J, Cn, score, seed=9) for f in range(off[-1])])
    out = tracks_np(p, x, off, score)
    for t in range(len(lengths)):
        want, _ = one_slot(x[off[t]:off[t + 1]], p, score) if lengths[t] else (np.zeros((0, J, x.shape[2]), np.float32), None)
        assert np.array_equal(bits(out[off[t]:off[t + 1]]), bits(want)), t


def test_the_two_statements_of_the_rule_agree_row_by_row():
    from tests.smooth_ref import push_rows_np
    J, Cn, score, S = 17, 2, True, 5
    p = params(min_score=0.3, max_hold=2)
    a, b = new_state(S, J, Cn, fill=-7.0), new_state(S, J, Cn, fill=-7.0)
    for i in range(14):
        slots = (None, np.array([3, 0]), np.array([1, 4, 3]))[i % 3]
        x = rows_for(i, S if slots is None else len(slots), J, Cn, score, seed=3)
        tick = i + (2 if i > 8 else 0)
        assert np.array_equal(bits(push_np(a, p, x, slots, tick, score)), bits(push_rows_np(b, p, x, slots, tick, score))), i
        assert all(np.array_equal(bits(a[k]) if a[k].dtype == np.float32 else a[k], bits(b[k]) if b[k].dtype == np.float32 else b[k]) for k in ("xhat", "dxhat", "last"))


# ---- sanity of the rule: not a speed or quality claim ----
def test_static_joint_with_noise_gets_steadier():
    g = np.random.default_rng(2012)
    x = np.zeros((300, 1, 3), np.float32)
    x[:, 0, :2] = (np.array([640.0, 360.0]) + g.normal(0.0, 2.0, (300, 2))).astype(np.float32)
    x[:, 0, 2] = 0.9
    out, _ = one_slot(x, params(), True)
    s_in, s_out = x[50:, 0, :2].std(0), out[50:, 0, :2].std(0)
    print(f"static joint, sigma = 2 px, defaults: input std {s_in}, output std {s_out}")
    assert (s_out < 0.5 * s_in).all()


# ---- the fp32 restatement against the fp64 one ----
def fp32_inputs():
    """300 ticks of 4 slots x 17 joints: a centre in [200, 800) px, a swing of up to 200 px with a period of 1 to 4 s, 2 px of noise, 30 % of the scores below
    min_score = 0.3: coordinates up to about 1,000 px."""
    g = np.random.default_rng(1204)
    n, S, J = 300, 4, 17
    t = np.arange(n)[:, None, None, None] / 30.0
    centre, amp = 200.0 + 600.0 * g.random((1, S, J, 2)), 200.0 * g.random((1, S, J, 2))
    x = np.zeros((n, S, J, 3), np.float32)
    x[..., :2] = (centre + amp * np.sin(2 * np.pi * t / (1.0 + 3.0 * g.random((1, S, J, 2)))) + g.normal(0.0, 2.0, (n, S, J, 2))).astype(np.float32)
    x[..., 2] = np.where(g.random((n, S, J)) < 0.3, 0.1, 0.9)
    return x


def test_fp32_restatement_against_fp64():
    x = fp32_inputs()
    p = params()
    s32, s64 = new_state(4, 17, 2), new_state(4, 17, 2, np.float64)
    err = 0.0
    for tick in range(len(x)):
        o32, o64 = push_np(s32, p, x[tick], None, tick, True), push_np(s64, p, x[tick], None, tick, True, np.float64)
        assert o32.dtype == np.float32 and o64.dtype == np.float64
        err = max(err, float(np.abs(o32 - o64).max()))
    assert np.array_equal(s32["last"], s64["last"])
    gated = float((x[..., 2] < 0.3).mean())
    print(f"fp32 against fp64 restatement: {err:.3g} px at coordinates up to {np.abs(x[..., :2]).max():.0f} px, {gated:.0%} gated (written into the test: "
          f"{FP32_MEASURED:.3g}, bar {FP32_BAR:.3g})")
    assert 0.25 < gated < 0.35 and 900.0 < np.abs(x[..., :2]).max() < 1100.0
    assert err <= FP32_BAR


# ---- refusals without a device ----
def test_parameter_refusals():
    from kasportsformer_amd.smooth import one_euro_params
    q = one_euro_params(30.0, 1.0, 0.01, 1.0, 0.3, 15)
    p = params()
    assert (np.float32(q.dt), q.min_cutoff, q.d_cutoff, np.float32(q.beta), np.float32(q.min_score), q.max_hold) == (p["dt"], 1.0, 1.0, p["beta"], p["min_score"], 15)
    for exc, kw in ((ValueError, dict(rate=0)), (ValueError, dict(rate=-30.0)), (ValueError, dict(rate=float("nan"))), (ValueError, dict(rate=float("inf"))),
                    (ValueError, dict(rate=1e7)), (ValueError, dict(rate=1e-7)), (ValueError, dict(min_cutoff=0.0)), (ValueError, dict(min_cutoff=1e7)),
                    (ValueError, dict(min_cutoff=float("nan"))), (ValueError, dict(d_cutoff=0.0)), (ValueError, dict(d_cutoff=2e6)), (ValueError, dict(beta=-0.1)),
                    (ValueError, dict(beta=2e6)), (ValueError, dict(beta=float("nan"))), (ValueError, dict(min_score=float("nan"))),
                    (ValueError, dict(min_score=float("inf"))), (ValueError, dict(max_hold=-1)), (ValueError, dict(max_hold=2 ** 20 + 1)),
                    (TypeError, dict(max_hold=1.5)), (TypeError, dict(max_hold=True)), (TypeError, dict(rate="30")), (TypeError, dict(beta=None)),
                    (TypeError, dict(min_cutoff=True))):
        with pytest.raises(exc):
            one_euro_params(**kw)
    assert one_euro_params(beta=0, min_score=-1.0, max_hold=0).max_hold == 0 and one_euro_params(max_hold=2 ** 20).max_hold == 2 ** 20


def test_constructor_refusals():
    import kasportsformer_amd as K
    from kasportsformer_amd.smooth import check_filter_args
    good = dict(slots=None, joints=17, channels=2, score=True, streams=None, track_slots=None, rows="persons", num_person=1)
    assert check_filter_args(**dict(good, slots=32)) == (False, 32, 17, 2, 3, None, None, None, None)
    assert check_filter_args(**dict(good, streams=2, track_slots=4, num_person=2)) == (True, 8, 17, 2, 3, 2, 4, 0, 2)
    assert check_filter_args(**dict(good, streams=2, track_slots=4, rows="tracks", channels=3, score=False)) == (True, 8, 17, 3, 3, 2, 4, 1, 4)
    for exc, kw in ((ValueError, dict()), (ValueError, dict(slots=4, streams=1)), (ValueError, dict(slots=4, track_slots=4)), (ValueError, dict(slots=0)),
                    (TypeError, dict(slots=4.0)), (TypeError, dict(slots=True)), (ValueError, dict(slots=4, joints=0)), (ValueError, dict(slots=4, joints=257)),
                    (ValueError, dict(slots=4, channels=0)), (ValueError, dict(slots=4, channels=5)), (TypeError, dict(slots=4, channels=2.0)),
                    (TypeError, dict(slots=4, score=1)), (ValueError, dict(streams=0, track_slots=4)), (ValueError, dict(streams=1, track_slots=0)),
                    (ValueError, dict(streams=1, track_slots=65)), (ValueError, dict(streams=1, track_slots=4, rows="people")),
                    (ValueError, dict(streams=1, track_slots=4, num_person=0)), (TypeError, dict(streams="1", track_slots=4))):
        with pytest.raises(exc):
            check_filter_args(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="OneEuroFilter"):
        K.OneEuroFilter(slots=4, device="cpu")
    with pytest.raises(ValueError, match="beta"):                  # the parameters are refused before the device is looked at
        K.OneEuroFilter(slots=4, beta=-1.0, device="cpu")


def test_push_and_reset_refusals():
    from kasportsformer_amd.smooth import check_push, check_slot_ids, check_stream_ids
    dev = torch.device("cuda", 0)
    f = SimpleNamespace(tracked=False, slots=4, joints=17, _Ct=3, streams=None, track_slots=None, R=None, device=dev)
    x = np.zeros((4, 17, 3), np.float32)
    xt, ids, fields, ticks = check_push(f, x, None, None, 1)
    assert tuple(xt.shape) == (4, 17, 3) and ids is None and fields is None and ticks == 1
    assert check_push(f, x[:2], None, [3, 1], 5)[1].tolist() == [3, 1]
    assert tuple(check_push(f, x[:0], None, [], 1)[0].shape) == (0, 17, 3)
    meta = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device="meta")      # noqa: E731
    t_ok = SimpleNamespace(ids=meta(2, 4), slot=meta(2, 4), born=meta(2, 4), count=meta(2))
    for exc, a in ((TypeError, (x.astype(np.float64), None, None, 1)), (TypeError, ([[0.0]], None, None, 1)), (ValueError, (x[:3], None, None, 1)),
                   (ValueError, (x[..., :2], None, None, 1)), (ValueError, (x, None, [0, 1], 1)), (ValueError, (x[:2], None, [0, 4], 1)),
                   (ValueError, (x[:2], None, [-1, 0], 1)), (ValueError, (x[:2], None, [1, 1], 1)), (ValueError, (x[:2], None, [[0, 1]], 1)),
                   (ValueError, (x[:2], None, [0.0, 1.0], 1)), (TypeError, (x, t_ok, None, 1)), (ValueError, (x, None, None, 0)), (TypeError, (x, None, None, 1.0)),
                   (TypeError, (x, None, None, True)), (RuntimeError, (torch.zeros((4, 17, 3), device="meta"), None, None, 1))):
        with pytest.raises(exc):
            check_push(f, *a)
    ft = SimpleNamespace(tracked=True, slots=8, joints=17, _Ct=3, streams=2, track_slots=4, R=2, device=torch.device("meta"))
    assert len(check_push(ft, np.zeros((2, 2, 17, 3), np.float32), t_ok, None, 1)[2]) == 4
    assert len(check_push(ft, np.zeros((4, 17, 3), np.float32), t_ok, None, 2)[2]) == 4
    for exc, a in ((TypeError, (np.zeros((4, 17, 3), np.float32), None, None, 1)), (TypeError, (np.zeros((4, 17, 3), np.float32), t_ok, [0], 1)),
                   (ValueError, (np.zeros((2, 17, 3), np.float32), t_ok, None, 1)), (ValueError, (np.zeros((2, 2, 17, 2), np.float32), t_ok, None, 1)),
                   (TypeError, (np.zeros((4, 17, 3), np.float32), object(), None, 1)),
                   (ValueError, (np.zeros((4, 17, 3), np.float32), SimpleNamespace(**dict(vars(t_ok), ids=meta(2, 5))), None, 1)),
                   (TypeError, (np.zeros((4, 17, 3), np.float32), SimpleNamespace(**dict(vars(t_ok), born=meta(2, 4, dtype=torch.int64))), None, 1))):
        with pytest.raises(exc):
            check_push(ft, *a)
    ft.device = dev
    with pytest.raises(RuntimeError):                              # the TrackResult is read in place: it must be on the filter's device
        check_push(ft, np.zeros((4, 17, 3), np.float32), t_ok, None, 1)
    assert check_slot_ids(None, 4, "w") is None and check_slot_ids(torch.tensor([2, 0]), 4, "w").dtype == np.int32
    assert check_stream_ids(None, 2, "w") is None and check_stream_ids(1, 2, "w") == [1] and check_stream_ids([0, 1], 2, "w") == [0, 1]
    for exc, v in ((ValueError, 2), (ValueError, [-1]), (TypeError, 0.5), (TypeError, [[0]]), (TypeError, "a")):
        with pytest.raises(exc):
            check_stream_ids(v, 2, "w")


def test_smooth_tracks_refusals():
    import kasportsformer_amd as K
    x = np.zeros((5, 17, 3), np.float32)
    for exc, a, kw in ((TypeError, x.astype(np.float64), {}), (TypeError, "x", {}), (TypeError, [x, x.astype(np.float16)], {}), (ValueError, x[0], {}),
                       (ValueError, [x, x[0]], {}), (ValueError, [x, x[..., :2]], {}), (ValueError, [x[None]], {}), (ValueError, np.zeros((1, 1, 5, 17, 3), np.float32), {}),
                       (ValueError, x[None], dict(offsets=[0, 5])), (ValueError, x, dict(offsets=[0, 4])), (ValueError, x, dict(offsets=[1, 5])),
                       (ValueError, x, dict(offsets=[0, 3, 2, 5])), (ValueError, x, dict(offsets=[0.0, 5.0])), (ValueError, x, dict(offsets=[])),
                       (ValueError, np.zeros((5, 17, 6), np.float32), {}), (ValueError, np.zeros((5, 17, 5), np.float32), dict(score=False)),
                       (ValueError, np.zeros((5, 17, 1), np.float32), {}), (ValueError, np.zeros((5, 300, 3), np.float32), {}), (TypeError, x, dict(score=1)),
                       (ValueError, x, dict(rate=0.0)), (ValueError, x, dict(max_hold=-1)), (ValueError, x, dict(beta=-1.0)),
                       (RuntimeError, x, dict(device="cpu"))):
        with pytest.raises(exc):
            K.smooth_tracks(a, **kw)
    assert K.smooth_tracks([]) == []


def _entry_args():
    from kasportsformer_amd import _lib
    q = _lib.KasfOneEuroParams(1.0 / 30.0, 1.0, 1.0, 0.01, 0.3, 15)
    return _lib.load(), q, 64                                      # 64: a non-null address that must never be dereferenced


def _bad_params():
    from kasportsformer_amd import _lib
    base = dict(dt=1.0 / 30.0, min_cutoff=1.0, d_cutoff=1.0, beta=0.01, min_score=0.3, max_hold=15)
    for kw in (dict(dt=0.0), dict(dt=1e-7), dict(dt=2e6), dict(dt=float("nan")), dict(min_cutoff=0.0), dict(min_cutoff=float("inf")), dict(d_cutoff=-1.0),
               dict(d_cutoff=2e6), dict(beta=-1e-3), dict(beta=2e6), dict(beta=float("nan")), dict(min_score=float("nan")), dict(min_score=float("-inf")),
               dict(max_hold=-1), dict(max_hold=2 ** 20 + 1)):
        yield kw, _lib.KasfOneEuroParams(**dict(base, **kw))


def test_entry_points_refuse_before_touching_a_pointer():
    lib, q, p = _entry_args()
    names = ["x", "slots", "K", "S", "J", "C", "has_score", "params", "tick", "xhat", "dxhat", "last", "out", "stream"]
    good = [p, p, 2, 4, 17, 2, 1, C.byref(q), 0, p, p, p, p, None]

    def call(fn, names, good, **kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)
    push = lib.kasf_one_euro_push
    for kw in (dict(J=0), dict(J=257), dict(C=0), dict(C=5), dict(K=-1), dict(S=-1), dict(K=5), dict(slots=None), dict(tick=-1), dict(params=None), dict(x=None),
               dict(xhat=None), dict(dxhat=None), dict(last=None), dict(out=None)):
        assert call(push, names, good, **kw) == 2, kw
        assert lib.kasf_last_error()
    for kw, bad in _bad_params():
        assert call(push, names, good, params=C.byref(bad)) == 2, kw
    assert call(push, names, good, K=0, x=None, xhat=None, dxhat=None, last=None, out=None, slots=None) == 0        # no rows: nothing to do
    assert call(push, names, good, K=0, J=0) == 2                                                                  # ... but the arguments are still checked
    names_t = ["x", "ids", "slot", "born", "count_b", "streams", "track_slots", "rows_mode", "R", "J", "C", "has_score", "params", "tick", "xhat", "dxhat", "last",
               "owner", "out", "row_slot", "stream"]
    good_t = [p, p, p, p, p, 2, 4, 0, 2, 17, 2, 1, C.byref(q), 0, p, p, p, p, p, None, None]
    tracked = lib.kasf_one_euro_tracked
    for kw in (dict(J=0), dict(J=257), dict(C=0), dict(C=5), dict(streams=0), dict(streams=-1), dict(track_slots=0), dict(track_slots=65), dict(R=0), dict(R=-2),
               dict(rows_mode=2), dict(rows_mode=-1), dict(streams=65536, R=65536), dict(tick=-1), dict(params=None), dict(x=None), dict(ids=None),
               dict(slot=None), dict(born=None), dict(count_b=None), dict(xhat=None), dict(dxhat=None), dict(last=None), dict(owner=None), dict(out=None)):
        assert call(tracked, names_t, good_t, **kw) == 2, kw
    for kw, bad in _bad_params():
        assert call(tracked, names_t, good_t, params=C.byref(bad)) == 2, kw
    names_r = ["x", "offsets", "N", "P", "J", "C", "has_score", "params", "out", "stream"]
    good_r = [p, p, 10, 2, 17, 2, 1, C.byref(q), p, None]
    tracks = lib.kasf_one_euro_tracks
    for kw in (dict(J=0), dict(J=257), dict(C=0), dict(C=5), dict(P=-1), dict(N=-1), dict(params=None), dict(x=None), dict(offsets=None), dict(out=None)):
        assert call(tracks, names_r, good_r, **kw) == 2, kw
    for kw, bad in _bad_params():
        assert call(tracks, names_r, good_r, params=C.byref(bad)) == 2, kw
    assert call(tracks, names_r, good_r, P=0, x=None, offsets=None, out=None) == 0
    assert call(tracks, names_r, good_r, P=0, C=5) == 2


# ---- the header, the build and the command line ----
def test_header_declares_the_entry_points_and_the_rule():
    from kasportsformer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "kasf.h")).read()
    declared = set(re.findall(r"\b(kasf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name, n_args in (("kasf_one_euro_push", 14), ("kasf_one_euro_tracked", 21), ("kasf_one_euro_tracks", 10)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for line in ("dtj  = float(k) * dt", "d    = (m - xhat) / dtj", "rd   = two_pi * d_cutoff * dtj", "ad   = rd / (rd + 1)", "dx   = dxhat + ad * (d - dxhat)",
                 "fc   = min_cutoff + beta * |dx|", "r    = two_pi * fc * dtj", "a    = r / (r + 1)", "xnew = xhat + a * (m - xhat)", "two_pi = 6.2831855f",
                 "k = max(tick - last[g][j], 1)", "k - 1 > max_hold", "owner[g] != id or born[b][r] != 0"):
        assert line in hdr, line
    assert lib.kasf_version() == _lib.ABI_VERSION == 12            # additive: the number did not change
    assert C.sizeof(_lib.KasfOneEuroParams) == 24
    mk = open(os.path.join(ROOT, "kasportsformer_amd", "csrc", "Makefile")).read()
    assert "k_smooth.hip" in mk and "$(BUILD)/k_smooth.o: EXTRA += -Rpass-analysis=kernel-resource-usage" in mk
    assert all("one_euro.h" in ln for ln in mk.splitlines() if ln.startswith("$(BUILD)/%.o:") or ln.startswith("build_asan/%.o:"))


def test_public_surface_and_command_line():
    import kasportsformer_amd as K
    from kasportsformer_amd.lift import _parse
    assert "OneEuroFilter" in K.__all__ and "smooth_tracks" in K.__all__ and "OneEuroFilter" in K.__doc__ and "not tuned" in K.OneEuroFilter.__doc__
    base = ["--config", "c.yaml", "--checkpoint", "b.pth", "--keypoints", "k.npy", "--width", "1280", "--height", "720", "--out", "o.npy"]
    a = _parse(base)
    assert a.smooth is False
    a = _parse(base + ["--smooth", "--smooth-rate", "25", "--smooth-min-cutoff", "0.5", "--smooth-beta", "0.02", "--smooth-min-score", "0.2", "--online"])
    assert (a.smooth, a.smooth_rate, a.smooth_min_cutoff, a.smooth_beta, a.smooth_min_score, a.online) == (True, 25.0, 0.5, 0.02, 0.2, True)
    with pytest.raises(SystemExit):
        _parse(base + ["--smooth-beta", "0.02"])                   # the parameters belong to --smooth
