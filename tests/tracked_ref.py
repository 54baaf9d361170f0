"""Shared by tests/test_tracked_cpu.py and tests/test_gpu_tracked.py (not a test): the tick rule of include/kasf.h (kasf_stream_track_front) in plain numpy over
hand-made ids / slot / born / count arrays, and the scripted sequence both files run.

The rule: row k of stream b takes track row r = count_b - 1 - k ("persons") or r = k ("tracks"), count_b clamped to [0, S_t]; the row is valid iff
k < min(count_b, R), id = ids[b, r] >= 1, s = slot[b, r] in [0, S_t) and no lower row of the stream that passes those tests has the same s.  A valid row with
owner[g] != id or born[b, r] != 0 (g = b * S_t + s) starts the slot again; then ring[g][count[g] % T] = frame, count[g] += 1."""
import numpy as np

WHY = ("ok", "past_count", "bad_id", "bad_slot", "duplicate")


def new_state(B, S_t, T, fill=0.0):
    return dict(ring=np.full((B * S_t, T, 17, 3), fill, np.float32), count=np.zeros(B * S_t, np.int64), owner=np.zeros(B * S_t, np.int32))


def tracked_front_np(state, track_arrays, rows, R, frames=None):
    """One tick.  ``state``: dict(ring [B*S_t,T,17,3], count [B*S_t], owner [B*S_t]), updated in place; ``track_arrays``: dict(ids, slot, born [B,S_t], count [B]);
    ``frames`` [B*R,17,3] (None: the ring is left alone).  Returns per row ``(row_slot int32 [B*R]: g or -1, reset bool [B*R], why: list of WHY strings)``."""
    ids, slot, born, count_b = (np.asarray(track_arrays[k]) for k in ("ids", "slot", "born", "count"))
    B, S_t = ids.shape
    T = state["ring"].shape[1]
    row_slot, reset, why = np.full(B * R, -1, np.int32), np.zeros(B * R, bool), []
    for b in range(B):
        cb = min(max(int(count_b[b]), 0), S_t)
        taken = set()
        for k in range(R):
            row = b * R + k
            if k >= cb:
                why.append("past_count")
                continue
            r = cb - 1 - k if rows == "persons" else k
            i, s = int(ids[b, r]), int(slot[b, r])
            if i < 1:
                why.append("bad_id")
                continue
            if not 0 <= s < S_t:
                why.append("bad_slot")
                continue
            if s in taken:
                why.append("duplicate")
                continue
            taken.add(s)
            why.append("ok")
            g = b * S_t + s
            if state["owner"][g] != i or born[b, r] != 0:
                state["count"][g], state["owner"][g], reset[row] = 0, i, True
            if frames is not None:
                state["ring"][g, state["count"][g] % T] = frames[row]
            state["count"][g] += 1
            row_slot[row] = g
    return row_slot, reset, why


def _arrays(per_stream, S_t, counts=None):
    """per_stream[b]: the emitted tracks newest first as (id, slot, born) -> padded TrackResult arrays (ids -1, slot 0, born 0 past the rows given)."""
    B = len(per_stream)
    ids, slot, born = np.full((B, S_t), -1, np.int32), np.zeros((B, S_t), np.int32), np.zeros((B, S_t), np.int32)
    count = np.zeros(B, np.int32)
    for b, rows in enumerate(per_stream):
        assert len(rows) <= S_t
        for r, (i, s, bn) in enumerate(rows):
            ids[b, r], slot[b, r], born[b, r] = i, s, bn
        count[b] = len(rows) if counts is None or counts[b] is None else counts[b]
    return dict(ids=ids, slot=slot, born=born, count=count)


def script(T, ticks, S_t=4):
    """Two streams of S_t = 4 tracker slots, per tick the TrackResult arrays.  An id keeps its slot (as the tracker's do), so a player's history can be kept
    per (stream, id) as well as per slot.
    Stream 0: id 1 on slot 0 in every tick (warm-up, then its ring wraps every T ticks); id 2 on slot 2 in ticks 1, 2 and 5 .. T + 1 (absent in 3, 4: its history
      goes on); from tick T + 2 slot 2 belongs to id 3, which arrives with born = 0 (only the owner table tells) and is flagged born = 1 once more at tick 2 T.
    Stream 1, by tick % 8: 0 nothing emitted; 1 one track; 2 four tracks with count 7 (clamped to 4); 3 the newer track's id is -1; 4 its slot is S_t (tick % 16
      == 12: -1); 5 a second track (id 9) claims slot 3 as well; 6, 7 two tracks: id 5 on slot 3 (newer) and id 1 on slot 1."""
    assert S_t == 4
    out = []
    for t in range(ticks):
        s0 = [(1, 0, 1 if t == 0 else 0)]
        if t in (1, 2) or 5 <= t < T + 2:
            s0.insert(0, (2, 2, 1 if t == 1 else 0))
        elif t >= T + 2:
            s0.insert(0, (3, 2, 1 if t == 2 * T else 0))
        C, D = (1, 1, 0), (5, 3, 0)
        m, cnt = t % 8, None
        if m == 0:
            s1 = []
        elif m == 1:
            s1 = [C]
        elif m == 2:
            s1, cnt = [D, C, (6, 0, 0), (7, 2, 0)], 7
        elif m == 3:
            s1 = [(-1, 3, 0), C]
        elif m == 4:
            s1 = [(5, -1 if t % 16 == 12 else S_t, 0), C]
        elif m == 5:
            s1 = [D, (9, 3, 0)]
        else:
            s1 = [D, C]
        out.append(_arrays([s0, s1], S_t, counts=[None, cnt]))
    return out


def frames_for(tick, n_rows, seed=0):
    """Synthetic keypoints [n_rows,17,3]: pixel x, y in [0, 1000), confidence in [0, 1)."""
    g = np.random.default_rng(1000 * seed + tick)
    f = g.random((n_rows, 17, 3), dtype=np.float32)
    f[..., :2] *= np.float32(1000.0)
    return f


class Cases:
    """What a run of the script has to contain; ``see`` is called once per tick with the owner table before and the state after it."""
    NAMES = ("warm_up", "two_wraps", "takeover", "born_same_id", "absent_then_back", "count_0", "count_1_of_2", "count_above_slots", "id_minus_1", "slot_outside",
             "duplicate")

    def __init__(self, T, S_t, R):
        self.T, self.S_t, self.R, self.seen, self.last_tick = T, S_t, R, set(), {}

    def see(self, tick, arrays, owner_before, owner_after, count_after, row_slot, reset, why):
        for cb in (int(c) for c in arrays["count"]):
            if cb == 0:
                self.seen.add("count_0")
            if cb == 1 and self.R >= 2:
                self.seen.add("count_1_of_2")
            if cb > self.S_t:
                self.seen.add("count_above_slots")
        for g, rs, w in zip(row_slot, reset, why):
            if w in ("bad_id", "bad_slot", "duplicate"):
                self.seen.add({"bad_id": "id_minus_1", "bad_slot": "slot_outside", "duplicate": "duplicate"}[w])
            if g < 0:
                continue
            i = int(owner_after[g])                    # the row's id
            if count_after[g] < self.T:
                self.seen.add("warm_up")
            if count_after[g] > 2 * self.T:
                self.seen.add("two_wraps")
            if rs and owner_before[g] not in (0, i):
                self.seen.add("takeover")
            if rs and owner_before[g] == i:
                self.seen.add("born_same_id")
            key = (int(g), i)
            if not rs and key in self.last_tick and self.last_tick[key] < tick - 1:
                self.seen.add("absent_then_back")
            self.last_tick[key] = tick

    def missing(self):
        return [n for n in self.NAMES if n not in self.seen]
