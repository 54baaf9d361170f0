"""The SORT tracker kernel (csrc/k_track.hip, K.SortTracker) against the dense numpy restatement of tests/test_track_cpu.py, tick by tick.

Held exact: ids, slot, born, count, dropped, person_count, the row order and the integer counters of ``state()``.  Held to a tolerance: x, P and the fp64
boxes of ``state()`` -- 64 x the largest difference between the dense BLAS / LAPACK restatement and the explicit-loop, no-FMA evaluation of the same rules
over these same sequences (x and boxes relative to the frame width, P relative to max |P|), floor 1e-12.  That difference was measured as 0.0 / 0.0
(tests/test_track_cpu.py, LOOP_VS_DENSE_*), so the floor is the tolerance: 1e-12 of 1280 pixels.  The fp32 boxes and persons: within one fp32 ulp of the
restatement's boxes rounded to fp32.

Not yet run on an MI355X when written (no GPU machine could be had); tests/test_track_host_cpu.py applies ``check_tick`` to the kernel's source compiled
for the host, where it is bit-equal to the restatement.
"""
import numpy as np
import pytest
import torch

from tests.test_heatmap_cpu import ulp_distance
from tests.test_track_cpu import (CASES, F32, FIXTURE_CASES, FRAME_W, LOOP_VS_DENSE_P, LOOP_VS_DENSE_X, fixture, pad, players, run_np)

pytestmark = pytest.mark.gpu

TOL_X = max(64 * LOOP_VS_DENSE_X, 1e-12)
TOL_P = max(64 * LOOP_VS_DENSE_P, 1e-12)
X_SCALE = np.array([FRAME_W, FRAME_W, FRAME_W * FRAME_W, 1.0, FRAME_W, FRAME_W, FRAME_W * FRAME_W])
STATE_INTS = (("ids", "id"), ("slot", "slot"), ("time_since_update", "tsu"), ("hits", "hits"), ("hit_streak", "streak"), ("age", "age"))


@pytest.fixture(scope="module")
def restated():
    """Every case through the restatement, once."""
    return {name: run_np(params, seq, states=True) for name, (params, seq, _) in CASES.items()}


def host(t):
    return t.cpu().numpy()


def run_gpu(params, dets, count, states=True, raw=False):
    """One stream of padded detections [T,rows,5] / count [T] through K.SortTracker -> per tick the TrackResult (and TrackState) as numpy, stream 0."""
    import kasportsformer_amd as K
    trk = K.SortTracker(streams=1, **params)
    d, c = torch.from_numpy(dets).cuda(), torch.from_numpy(count).cuda()
    out = []
    for t in range(len(dets)):
        r = trk.update(d[t:t + 1], c[t:t + 1])
        tick = {k: host(getattr(r, k))[0] for k in r._fields}
        if states:
            s = trk.state()
            tick["state"] = {k: host(getattr(s, k))[0] for k in s._fields}
        out.append(tick)
    return (out, trk) if raw else out


def check_tick(got, want, where):
    n = want["count"]
    for k in ("count", "dropped", "person_count"):
        assert int(got[k]) == want[k], (where, k, int(got[k]), want[k])
    for k in ("ids", "slot", "born"):
        assert np.array_equal(got[k][:n], want[k]), (where, k, got[k][:n], want[k])
    assert (got["ids"][n:] == -1).all() and not got["slot"][n:].any() and not got["born"][n:].any() and not got["boxes"][n:].any(), where
    if n:
        assert ulp_distance(got["boxes"][:n], want["boxes"].astype(F32)).max() <= 1, where
    pc = want["person_count"]
    assert not got["persons"][pc:].any(), where
    if pc:
        assert ulp_distance(got["persons"][:pc], want["persons"].astype(F32)).max() <= 1, where
    if "state" in got:
        gs, ws = got["state"], want["state"]
        m = ws["tracks"]
        for k in ("tracks", "next_id", "ticks"):
            assert int(gs[k]) == ws[k], (where, k)
        for gk, wk in STATE_INTS:
            assert np.array_equal(gs[gk][:m], ws[wk]) and not gs[gk][m:].any(), (where, gk)
        assert not gs["x"][m:].any() and not gs["P"][m:].any() and not gs["boxes"][m:].any(), where
        if m:
            ex = float((np.abs(gs["x"][:m] - ws["x"]) / X_SCALE).max())
            eb = float(np.abs(gs["boxes"][:m] - ws["boxes"]).max() / FRAME_W)
            ep = float(np.abs(gs["P"][:m] - ws["P"]).max() / np.abs(ws["P"]).max())
            assert ex <= TOL_X and eb <= TOL_X and ep <= TOL_P, (where, ex, eb, ep)
            return max(ex, eb), ep
    return 0.0, 0.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_follows_the_restatement_tick_by_tick(name, restated):
    params, seq, rows = CASES[name]
    dets, count = pad(seq, rows)
    got = run_gpu(params, dets, count)
    worst = (0.0, 0.0)
    for t, (g, w) in enumerate(zip(got, restated[name])):
        e = check_tick(g, w, (name, t))
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    print(f"{name}: x / boxes within {worst[0]:.3e} of the frame width, P within {worst[1]:.3e} of max |P|")


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_fixture_sequences_give_the_references_ids_and_order(name):
    z = fixture()
    params = CASES[name][0]
    got = run_gpu(params, z[f"{name}_dets"], z[f"{name}_count"], states=False)
    ret, ret_n = z[f"{name}_ret"], z[f"{name}_ret_count"]
    for t, g in enumerate(got):
        n = int(ret_n[t])
        assert int(g["count"]) == n, (name, t)
        assert np.array_equal(g["ids"][:n], ret[t, :n, 4].astype(np.int32)), (name, t)
        if n:
            assert np.abs(g["boxes"][:n].astype(np.float64) - ret[t, :n, :4]).max() <= 1e-3, (name, t)      # fp32 rows of a 1280-pixel frame


def bytes_of(ticks):
    return [tuple(np.ascontiguousarray(v).tobytes() for k, v in sorted(tick.items()) if k != "state") for tick in ticks]


def test_two_runs_give_the_same_bytes():
    params, seq, rows = CASES["default"]
    dets, count = pad(seq, rows)
    (a, ta), (b, tb) = run_gpu(params, dets, count, states=False, raw=True), run_gpu(params, dets, count, states=False, raw=True)
    assert bytes_of(a) == bytes_of(b)
    assert torch.equal(ta._state, tb._state)


def test_a_stream_of_a_batch_equals_the_stream_alone_and_reset():
    import kasportsformer_amd as K
    params = dict(slots=8, min_hits=1, max_age=2, num_person=2)
    padded = [pad(players(seed, people, ticks=20), 8) for seed, people in ((21, 3), (22, 5), (23, 1))]
    dets = np.stack([p[0] for p in padded], axis=1)                  # [T,3,8,5]
    count = np.stack([p[1] for p in padded], axis=1)
    trk = K.SortTracker(streams=3, **params)
    d, c = torch.from_numpy(dets).cuda(), torch.from_numpy(count).cuda()
    batch = []
    for t in range(len(dets)):
        r = trk.update(d[t], c[t])
        batch.append({k: host(getattr(r, k)) for k in r._fields})
    for b in range(3):
        alone, one = run_gpu(params, np.ascontiguousarray(dets[:, b]), np.ascontiguousarray(count[:, b]), states=False, raw=True)
        assert bytes_of(alone) == bytes_of([{k: v[b] for k, v in tick.items()} for tick in batch]), b
        assert torch.equal(one._state[0], trk._state[b]), b
    # reset of one stream: its ids start again, the others go on
    before = host(trk.state().next_id)
    trk.reset(1)
    assert not trk._state[1].any() and trk._state[0].any()
    r = trk.update(d[0], c[0])
    s = trk.state()
    assert host(s.ticks).tolist() == [21, 1, 21] and host(s.next_id)[1] == count[0, 1] and host(s.next_id)[0] >= before[0]
    assert sorted(host(r.ids)[1][:count[0, 1]].tolist()) == list(range(1, count[0, 1] + 1)), "the first tick of a fresh stream emits every birth, ids from 1"
    trk.reset()
    assert not trk._state.any()


def test_strided_views_and_host_input_equal_the_packed_copy():
    import kasportsformer_amd as K
    params, seq, rows = CASES["demo"]
    dets, _ = pad(seq, rows)
    seq = [dets[t, :len(s)] for t, s in enumerate(seq)]
    big = torch.full((1, 2 * rows, 14), 7.0, device="cuda")
    trackers = [K.SortTracker(**params) for _ in range(4)]
    for t, s in enumerate(seq):
        n = len(s)
        packed = torch.from_numpy(np.ascontiguousarray(s)).cuda()
        big[0, 0:2 * n:2, 3:8] = packed
        big[0, :n, 9:14] = packed
        wide = big[:, 0:2 * n:2, 3:8]                                 # a row stride of 28 elements, adjacent columns: read in place
        assert wide.stride(2) == 1 and (n < 2 or not wide.is_contiguous())
        spread = torch.empty((1, n, 10), device="cuda")
        spread[:, :, ::2] = packed
        res = [trackers[0].update(packed[None]), trackers[1].update(wide), trackers[2].update(spread[:, :, ::2]), trackers[3].update(s)]     # s: numpy [n,5] on the host
        for r in res[1:]:
            assert all(torch.equal(a, b) for a, b in zip(res[0], r)), t
    assert all(torch.equal(trackers[0]._state, k._state) for k in trackers[1:])
    assert (big[0, :, :3] == 7).all() and (big[0, :, 8] == 7).all(), "the input is not written"


def test_detector_to_tracker_to_crop_stays_on_the_device():
    import kasportsformer_amd as K
    pred = torch.zeros((1, 16, 85))
    boxes = [(100.0, 200.0, 60.0, 150.0), (300.0, 180.0, 70.0, 160.0)]
    for k, (cx, cy, w, h) in enumerate(boxes):
        pred[0, 3 * k + 1, :5] = torch.tensor([cx, cy, w, h, 0.9 - 0.1 * k])
        pred[0, 3 * k + 1, 5] = 0.95
    pred = pred.cuda()
    frame = torch.randint(0, 256, (416, 416, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    trk = K.SortTracker(min_hits=0, num_person=2)
    side = torch.full((1,), 416.0, device="cuda")                   # the frame's size as a GPU tensor: a host number would be uploaded, which synchronises
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                          # a synchronising torch call between the three stages raises
    try:
        r = K.detections_to_boxes(pred, side, side, inp_dim=416)
        t = trk.update(r.boxes, r.count)
        crops = K.crop_persons(frame, t.persons[0], size=(48, 64))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert tuple(crops.inputs.shape) == (2, 3, 64, 48) and torch.isfinite(crops.inputs).all()
    n = int(r.count[0])
    assert n == 2 and int(t.count[0]) == 2 and int(t.person_count[0]) == 2 and host(t.ids)[0, :2].tolist() == [2, 1] and host(t.born)[0, :2].tolist() == [1, 1]
    # a new track's box is the detection's through z and back: newest first, persons oldest first
    want = host(r.boxes)[0, :2, :4]
    assert np.abs(host(t.persons)[0] - want).max() <= 1e-3 and np.abs(host(t.boxes)[0, :2] - want[::-1]).max() <= 1e-3
    alone = K.crop_persons(frame, r.boxes[0, :2, :4], size=(48, 64))
    assert (crops.inputs - alone.inputs).abs().max() <= 0.5          # the same two people, boxes equal to 1e-3 pixels


def test_entry_point_refuses_device_pointers_too():
    from kasportsformer_amd import _lib
    from tests.gpu_util import ptr, stream
    lib = _lib.load()
    state = torch.full((lib.kasf_sort_state_bytes(1, 4, 8),), 3, dtype=torch.uint8, device="cuda")
    dets, out = torch.zeros((1, 8, 5), device="cuda"), torch.full((16,), 7.0, device="cuda")
    ints = torch.full((7, 4), 9, dtype=torch.int32, device="cuda")

    def call(slots=4, max_dets=8, det_rows=8, rstride=5, num_person=1):
        return lib.kasf_sort_update(ptr(state), 1, slots, max_dets, ptr(dets), det_rows, 40, rstride, None, 1, 3, 0.3, num_person, 0, ptr(out), ptr(ints[0]),
                                    ptr(ints[1]), ptr(ints[2]), ptr(ints[3]), ptr(ints[4]), ptr(out), ptr(ints[5]), stream())

    for kw in (dict(slots=65), dict(max_dets=65), dict(det_rows=9), dict(rstride=3), dict(num_person=0)):
        assert call(**kw) == 2, kw
    torch.cuda.synchronize()
    assert (state == 3).all() and (out == 7).all() and (ints == 9).all(), "a refused call launches nothing"
