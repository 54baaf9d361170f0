"""Host side of the tracked lifter (kasportsformer_amd.TrackedLifter, kasf_stream_track_front / _emit): the numpy restatement of the tick rule
(tests/tracked_ref.py) against a second statement of it that keeps one list of frames per player, the refusals of the Python surface and of the two entry
points without a device, and the header."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.tracked_ref import Cases, frames_for, new_state, script, tracked_front_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _second_statement(arrays, rows, R, S_t, players, holder, frames):
    """The rule once more, told per player: ``players[(stream, id)]`` is the list of frames of that player's current history, ``holder[(stream, slot)]`` the
    id the slot last served.  Validity is worked out over whole streams with array operations.  Returns per row (stream, id, whether a history began) or None."""
    B = arrays["ids"].shape[0]
    out = []
    for b in range(B):
        cb = int(np.clip(arrays["count"][b], 0, S_t))
        k = np.arange(R)
        r = np.clip(cb - 1 - k if rows == "persons" else k, 0, S_t - 1)
        i, s, bn = arrays["ids"][b][r], arrays["slot"][b][r], arrays["born"][b][r]
        cand = (k < cb) & (i >= 1) & (s >= 0) & (s < S_t)
        first = np.zeros(R, bool)
        for sv in np.unique(s[cand]):
            first[np.flatnonzero(cand & (s == sv))[0]] = True
        for kk in range(R):
            if not first[kk]:
                out.append(None)
                continue
            key = (b, int(i[kk]))
            fresh = holder.get((b, int(s[kk]))) != key[1] or bn[kk] != 0
            if fresh:
                players[key] = []
                holder[(b, int(s[kk]))] = key[1]
            players[key].append(frames[b * R + kk])
            out.append(key + (fresh,))
    return out


@pytest.mark.parametrize("rows,R", [("persons", 2), ("tracks", 4)])
@pytest.mark.parametrize("T", [5, 27])
def test_restatement_against_the_per_player_statement(T, rows, R):
    B, S_t, ticks = 2, 4, 3 * T + 4
    state, players, holder, cases = new_state(B, S_t, T, fill=-1.0), {}, {}, Cases(T, S_t, R)
    for tick, arrays in enumerate(script(T, ticks)):
        fr = frames_for(tick, B * R, seed=T)
        owner_before = state["owner"].copy()
        untouched = {k: v.copy() for k, v in state.items()}
        row_slot, reset, why = tracked_front_np(state, arrays, rows, R, fr)
        keys = _second_statement(arrays, rows, R, S_t, players, holder, fr)
        cases.see(tick, arrays, owner_before, state["owner"], state["count"], row_slot, reset, why)
        assert [w == "ok" for w in why] == [k is not None for k in keys] == (row_slot >= 0).tolist(), tick
        touched = set()
        for row, key in enumerate(keys):
            if key is None:
                assert not reset[row]
                continue
            g = int(row_slot[row])
            b, i, fresh = key
            touched.add(g)
            assert g // S_t == b and state["owner"][g] == i, (tick, row)
            hist = players[(b, i)]
            assert state["count"][g] == len(hist) and bool(reset[row]) == fresh, (tick, row)
            n = len(hist)
            for c in range(max(0, n - T), n):                      # the window's frames, where the ring keeps them
                assert np.array_equal(state["ring"][g, c % T], hist[c]), (tick, row, c)
        for g in range(B * S_t):                                   # nothing else moved
            if g not in touched:
                assert state["count"][g] == untouched["count"][g] and state["owner"][g] == untouched["owner"][g]
                assert np.array_equal(state["ring"][g], untouched["ring"][g])
    assert not cases.missing(), cases.missing()


def test_check_tracked_args_refusals():
    from kasportsformer_amd.tracked import check_tracked_args, check_tracked_frames, check_tracked_tick
    good = dict(T=27, width=1280, height=720, streams=2, track_slots=4, rows="persons", num_person=2, lag=0, layout="h36m")
    T, w, h, B, S_t, mode, R, lag, coco = check_tracked_args(**good)
    assert (T, B, S_t, mode, R, lag, coco) == (27, 2, 4, 0, 2, 0, False) and w.dtype == np.float32 and w.tolist() == [1280.0, 1280.0] and h.tolist() == [720.0] * 2
    assert check_tracked_args(**dict(good, rows="tracks", layout="coco", width=[640, 1920], lag=26))[3:] == (2, 4, 1, 4, 26, True)
    for exc, kw in ((ValueError, dict(lag=-1)), (ValueError, dict(lag=27)), (ValueError, dict(rows="people")), (ValueError, dict(rows=None)),
                    (ValueError, dict(layout="openpose")), (ValueError, dict(width=0)), (ValueError, dict(height=-720)), (ValueError, dict(width=[1280, 0])),
                    (ValueError, dict(width=[1280] * 3)), (ValueError, dict(streams=0)), (ValueError, dict(track_slots=0)), (ValueError, dict(track_slots=65)),
                    (ValueError, dict(num_person=0)), (TypeError, dict(streams=2.0)), (TypeError, dict(track_slots="4")), (ValueError, dict(T=0))):
        with pytest.raises(exc):
            check_tracked_args(**dict(good, **kw))
    dev = torch.device("cuda", 0)
    meta = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device="meta")      # noqa: E731
    t_ok = SimpleNamespace(ids=meta(2, 4), slot=meta(2, 4), born=meta(2, 4), count=meta(2))
    for exc, t in ((ValueError, SimpleNamespace(**dict(vars(t_ok), ids=meta(2, 5)))), (ValueError, SimpleNamespace(**dict(vars(t_ok), count=meta(3)))),
                   (ValueError, SimpleNamespace(**dict(vars(t_ok), slot=meta(1, 4)))), (TypeError, SimpleNamespace(**dict(vars(t_ok), born=meta(2, 4, dtype=torch.int64)))),
                   (TypeError, SimpleNamespace(**dict(vars(t_ok), count=[1, 2]))), (TypeError, object()),
                   (RuntimeError, t_ok),                                                         # not on the lifter's device
                   (RuntimeError, SimpleNamespace(**{k: torch.zeros(v.shape, dtype=torch.int32) for k, v in vars(t_ok).items()}))):
        with pytest.raises(exc):
            check_tracked_tick(t, 2, 4, dev)
    assert len(check_tracked_tick(t_ok, 2, 4, torch.device("meta"))) == 4
    check_tracked_frames(torch.empty((2, 2, 17, 3)), 2, 2)
    check_tracked_frames(torch.empty((4, 17, 3)), 2, 2)
    for shape in ((2, 17, 3), (2, 2, 17, 2), (1, 4, 17, 3), (4, 51)):
        with pytest.raises(ValueError):
            check_tracked_frames(torch.empty(shape), 2, 2)


def test_tracked_lifter_needs_a_gpu_model():
    import kasportsformer_amd as K
    m = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=27, compute_dtype="fp32")
    with pytest.raises(RuntimeError, match="TrackedLifter"):
        K.TrackedLifter(m, 1280, 720, streams=1, track_slots=4)
    assert K.TrackedTick._fields == ("poses", "valid", "ids", "frames")


def test_entry_points_refuse_before_touching_a_pointer():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    p = 64                                                   # a non-null address that must never be dereferenced
    front = lib.kasf_stream_track_front
    # (frames, ids, slot, born, count_b, streams, track_slots, rows_mode, R, T, ring, count, owner, width, height, resample_tab, flip, x, row_slot, stream)
    good = [p, p, p, p, p, 2, 4, 0, 2, 27, p, p, p, p, p, p, 1, p, p, None]

    def with_(**kw):
        names = ["frames", "ids", "slot", "born", "count_b", "streams", "track_slots", "rows_mode", "R", "T", "ring", "count", "owner", "width", "height",
                 "resample_tab", "flip", "x", "row_slot", "stream"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a
    for kw in (dict(streams=0), dict(streams=-1), dict(track_slots=0), dict(track_slots=65), dict(track_slots=-4), dict(R=0), dict(R=-2), dict(T=0), dict(T=257),
               dict(rows_mode=2), dict(rows_mode=-1), dict(streams=65536, R=65536), dict(frames=None), dict(ids=None), dict(slot=None), dict(born=None),
               dict(count_b=None), dict(ring=None), dict(count=None), dict(owner=None), dict(width=None), dict(height=None), dict(resample_tab=None),
               dict(x=None), dict(row_slot=None)):
        assert front(*with_(**kw)) == 2, kw
        assert lib.kasf_last_error()
    assert front(*([None] * 5 + [2, 4, 0, 2, 27] + [None] * 6 + [1, None, None, None])) == 2
    emit = lib.kasf_stream_track_emit
    # (pred, flip, count, owner, row_slot, n_rows, T, first_pos_tab, back, out, valid, ids_out, frames_out, stream)
    good_e = [p, 1, p, p, p, 4, 27, p, 0, p, p, p, p, None]
    for idx, v in ((6, 0), (6, 257), (8, -1), (8, 27), (5, -1), (0, None), (2, None), (3, None), (4, None), (7, None), (9, None), (10, None), (11, None),
                   (12, None)):
        a = list(good_e)
        a[idx] = v
        assert emit(*a) == 2, (idx, v)
    assert emit(None, 1, None, None, None, 0, 27, None, 0, None, None, None, None, None) == 0         # no rows: nothing to do
    assert emit(None, 1, None, None, None, 0, 27, None, 27, None, None, None, None, None) == 2        # ... but the arguments are still checked


def test_header_declares_the_entry_points_and_the_rule():
    from kasportsformer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "kasf.h")).read()
    declared = set(re.findall(r"\b(kasf_[a-z0-9_]+)\s*\(", hdr))
    for name in ("kasf_stream_track_front", "kasf_stream_track_emit"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert "#define KASF_ROWS_PERSONS 0" in hdr and "#define KASF_ROWS_TRACKS 1" in hdr
    assert (_lib.ROWS_PERSONS, _lib.ROWS_TRACKS) == (0, 1)
    assert "owner[g] != id or born[b][r] != 0" in hdr and "r = count_b - 1 - k" in hdr, "the tick rule is stated in the header"
    assert _lib.load().kasf_version() == _lib.ABI_VERSION == 12
