"""The tracked lifter on the GPU (kasportsformer_amd.TrackedLifter, csrc/k_stream_track.hip): the front kernel against the numpy restatement of the tick
rule (tests/tracked_ref.py) and, for its clips, bit for bit against the existing kasf_stream_windows on the same state; the emit kernel against the existing
kasf_stream_emit; the class against a plain StreamLifter driven from the host as the restatement dictates (fp32, exact), against its own parts (bf16), behind
the real tracker, with COCO frames and heatmaps, without a host synchronisation, and from run to run.

Not yet run on an MI355X when written (no GPU machine could be had); tests/test_tracked_host_cpu.py applies the front and emit checks to the kernels' source
compiled for the host, where it is bit-equal to the restatements.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.tracked_ref import Cases, frames_for, new_state, script, tracked_front_np

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, S_T = 2, 4
RES = [(1280, 720), (1437, 913)]                       # one resolution per stream
CANARY = 12345.5


def _dev(arrays):
    """TrackResult-like arrays on the device."""
    return SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()})


def _tables(T):
    from kasportsformer_amd.stream import stream_tables
    r, fp = stream_tables(T)
    return torch.from_numpy(r).cuda(), torch.from_numpy(fp).cuda()


def _wh(per_slot):
    n = S_T if per_slot else 1
    return (torch.tensor([RES[b][0] for b in range(B) for _ in range(n)], dtype=torch.float32, device="cuda"),
            torch.tensor([RES[b][1] for b in range(B) for _ in range(n)], dtype=torch.float32, device="cuda"))


class _FrontRun:
    """The front kernel on a state of its own, with canaries around ring and behind x (x starts one float into its buffer: clips at every alignment)."""

    def __init__(self, T, rows, R, flip):
        self.T, self.rows, self.R, self.flip, self.halves, self.n = T, rows, R, flip, (2 if flip else 1), B * R
        self.mode = 0 if rows == "persons" else 1
        ring_floats = B * S_T * T * 51
        self.ring_buf = torch.full((ring_floats + 128,), CANARY, device="cuda")
        self.ring = self.ring_buf[64:64 + ring_floats].view(B * S_T, T, 17, 3)
        self.ring.fill_(-1.0)
        self.count = torch.zeros(B * S_T, dtype=torch.int64, device="cuda")
        self.owner = torch.zeros(B * S_T, dtype=torch.int32, device="cuda")
        self.x_floats = self.halves * self.n * T * 51
        self.x_buf = torch.empty(self.x_floats + 65, device="cuda")
        self.r_tab, self.fp_tab = _tables(T)
        self.w, self.h = _wh(False)

    def tick(self, arrays, frames_d):
        from kasportsformer_amd import _lib
        t = _dev(arrays)
        self.x_buf.fill_(CANARY)
        x = self.x_buf[1:1 + self.x_floats].view(self.halves * self.n, self.T, 17, 3)
        row_slot = torch.full((self.n,), -7, dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().kasf_stream_track_front(ptr(frames_d), ptr(t.ids), ptr(t.slot), ptr(t.born), ptr(t.count), B, S_T, self.mode, self.R, self.T,
                                                       ptr(self.ring), ptr(self.count), ptr(self.owner), ptr(self.w), ptr(self.h), ptr(self.r_tab),
                                                       int(self.flip), ptr(x), ptr(row_slot), stream()))
        torch.cuda.synchronize()
        return x, row_slot

    def canaries_intact(self):
        return bool((self.ring_buf[:64] == CANARY).all() and (self.ring_buf[-64:] == CANARY).all() and self.x_buf[0] == CANARY
                    and (self.x_buf[1 + self.x_floats:] == CANARY).all())


def _windows_of(run, slots):
    """What the existing kasf_stream_windows writes for these slots of the run's state (a copy of it)."""
    from kasportsformer_amd import _lib
    K = len(slots)
    ring, count = run.ring.clone(), run.count.clone()
    w, h = _wh(True)
    ids = torch.tensor(slots, dtype=torch.int32, device="cuda")
    x = torch.full((run.halves * K, run.T, 17, 3), float("nan"), device="cuda")
    _lib.check(_lib.load().kasf_stream_windows(ptr(ring), ptr(count), ptr(ids), K, B * S_T, run.T, ptr(w), ptr(h), ptr(run.r_tab), int(run.flip), ptr(x), stream()))
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("rows,R", [("persons", 2), ("tracks", 4)])
@pytest.mark.parametrize("T", [5, 27])
def test_front_kernel_follows_the_rule_and_writes_stream_windows_clips(T, rows, R, flip):
    run, state, cases = _FrontRun(T, rows, R, flip), new_state(B, S_T, T, fill=-1.0), Cases(T, S_T, R)
    n = B * R
    for tick, arrays in enumerate(script(T, 3 * T + 4)):
        fr = frames_for(tick, n, seed=T)
        fr_d = torch.from_numpy(fr).cuda()
        owner_before = state["owner"].copy()
        want_slot, reset, why = tracked_front_np(state, arrays, rows, R, fr)
        cases.see(tick, arrays, owner_before, state["owner"], state["count"], want_slot, reset, why)
        x, row_slot = run.tick(arrays, fr_d)
        assert np.array_equal(row_slot.cpu().numpy(), want_slot), (tick, row_slot.tolist(), want_slot.tolist())
        assert np.array_equal(run.count.cpu().numpy(), state["count"]), tick
        assert np.array_equal(run.owner.cpu().numpy(), state["owner"]), tick
        assert np.array_equal(run.ring.cpu().numpy(), state["ring"]), tick
        assert np.array_equal(fr_d.cpu().numpy(), fr), tick
        assert run.canaries_intact(), tick
        valid = [r for r in range(n) if want_slot[r] >= 0]
        if valid:
            xw = _windows_of(run, [int(want_slot[r]) for r in valid])
            for h in range(run.halves):
                for i, r in enumerate(valid):
                    assert torch.equal(x[h * n + r], xw[h * len(valid) + i]), (tick, h, r)
        for h in range(run.halves):
            for r in range(n):
                if want_slot[r] < 0:
                    assert not x[h * n + r].any(), (tick, h, r)
    assert not cases.missing(), cases.missing()


@pytest.mark.parametrize("flip", [True, False])
@pytest.mark.parametrize("T", [5, 27])
def test_emit_kernel_is_stream_emit_on_the_valid_rows(T, flip):
    from kasportsformer_amd import _lib
    lib = _lib.load()
    S, halves = B * S_T, (2 if flip else 1)
    r_tab, fp_tab = _tables(T)
    count = torch.tensor([1, 2, T - 1, T, T + 1, 2 * T + 3, 0, 3 * T + 5], dtype=torch.int64, device="cuda")
    owner = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6], dtype=torch.int32, device="cuda")
    row_slot_np = np.array([5, -1, 0, 3, -1, 7, 2, 4, 1], np.int32)
    n = len(row_slot_np)
    row_slot = torch.from_numpy(row_slot_np).cuda()
    pred = torch.randn((halves * n, T, 17, 3), generator=torch.Generator().manual_seed(T + flip)).cuda()
    valid_rows = [r for r in range(n) if row_slot_np[r] >= 0]
    K = len(valid_rows)
    idx = torch.tensor(valid_rows + ([n + r for r in valid_rows] if flip else []), device="cuda")
    pred_k, ids_k = pred[idx].contiguous(), torch.from_numpy(row_slot_np[valid_rows]).cuda()
    for back in sorted({0, min(3, T - 1), T - 1}):
        out = torch.full((n, 17, 3), float("nan"), device="cuda")
        valid = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        ids_out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        frames_out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        _lib.check(lib.kasf_stream_track_emit(ptr(pred), int(flip), ptr(count), ptr(owner), ptr(row_slot), n, T, ptr(fp_tab), back, ptr(out), ptr(valid),
                                              ptr(ids_out), ptr(frames_out), stream()))
        want = torch.full((K, 1, 17, 3), float("nan"), device="cuda")
        _lib.check(lib.kasf_stream_emit(ptr(pred_k), int(flip), ptr(count), ptr(ids_k), K, S, T, ptr(fp_tab), back, 1, ptr(want), stream()))
        torch.cuda.synchronize()
        for i, r in enumerate(valid_rows):
            assert torch.equal(out[r], want[i, 0]), (back, r)
        for r in range(n):
            g = int(row_slot_np[r])
            if g < 0:
                assert not out[r].any() and valid[r] == 0 and ids_out[r] == 0 and frames_out[r] == 0, (back, r)
            else:
                assert valid[r] == 1 and ids_out[r] == owner[g] and frames_out[r] == count[g], (back, r)


_MODELS = {}


def _model(cd):
    if cd not in _MODELS:
        _MODELS[cd] = make_pair(1, 27, cd)[1].eval()
    return _MODELS[cd]


def _lifter(cd="fp32", **kw):
    import kasportsformer_amd as K
    args = dict(streams=B, track_slots=S_T, rows="persons", num_person=2)
    args.update(kw)
    return K.TrackedLifter(_model(cd), [RES[b][0] for b in range(B)], [RES[b][1] for b in range(B)], **args)


def _check_against_plain_lifter(lag, ticks=59):
    """The class against StreamLifter(slots=8) driven from the host by the restatement; returns the poses of every tick."""
    import kasportsformer_amd as K
    T, R = 27, 2
    n = B * R
    lifter = _lifter(lag=lag)
    plain = K.StreamLifter(_model("fp32"), [RES[g // S_T][0] for g in range(B * S_T)], [RES[g // S_T][1] for g in range(B * S_T)], slots=B * S_T, lag=lag)
    state, cases, poses = new_state(B, S_T, T), Cases(T, S_T, R), []
    for tick, arrays in enumerate(script(T, ticks)):
        fr = frames_for(tick, n, seed=7)
        owner_before = state["owner"].copy()
        row_slot, reset, why = tracked_front_np(state, arrays, "persons", R, fr)
        cases.see(tick, arrays, owner_before, state["owner"], state["count"], row_slot, reset, why)
        out = lifter.push(torch.from_numpy(fr).cuda().view(B, R, 17, 3) if tick % 2 else fr, _dev(arrays))
        assert out.poses.dtype == torch.float32 and tuple(out.poses.shape) == (B, R, 17, 3) and out.poses.grad_fn is None
        assert out.valid.dtype == torch.bool and out.ids.dtype == torch.int32 and out.frames.dtype == torch.int64
        valid = [r for r in range(n) if row_slot[r] >= 0]
        if reset.any():
            plain.reset(slots=[int(row_slot[r]) for r in range(n) if reset[r]])
        got = out.poses.view(n, 17, 3)
        if valid:
            want = plain.push(fr[valid], slots=[int(row_slot[r]) for r in valid])
            for i, r in enumerate(valid):
                assert torch.equal(got[r], want[i]), (tick, r)
        assert out.valid.view(-1).cpu().tolist() == [r in valid for r in range(n)], tick
        assert out.ids.view(-1).cpu().tolist() == [int(state["owner"][row_slot[r]]) if r in valid else 0 for r in range(n)], tick
        assert out.frames.view(-1).cpu().tolist() == [int(state["count"][row_slot[r]]) if r in valid else 0 for r in range(n)], tick
        for r in range(n):
            if r not in valid:
                assert not got[r].any(), (tick, r)
        poses.append(got.clone())
    assert not cases.missing(), cases.missing()
    assert np.array_equal(lifter._count.cpu().numpy(), state["count"]) and np.array_equal(lifter._owner.cpu().numpy(), state["owner"])
    return poses, lifter._ring.clone()


@pytest.mark.parametrize("lag", [0, 5])
def test_class_equals_a_plain_stream_lifter_driven_from_the_host(lag):
    _check_against_plain_lifter(lag)


def test_bf16_tick_equals_its_parts():
    """One tick = front kernel -> _forward_windows -> emit kernel, bit for bit, on a warmed state (three ticks, each compared)."""
    from kasportsformer_amd import _lib
    from kasportsformer_amd.lift import _forward_windows
    lib, T, R = _lib.load(), 27, 2
    n = B * R
    lifter = _lifter("bf16", lag=2)
    for tick, arrays in enumerate(script(T, 8)[5:8]):
        fr_d, t = torch.from_numpy(frames_for(tick, n, seed=3)).cuda(), _dev(arrays)
        ring, count, owner = lifter._ring.clone(), lifter._count.clone(), lifter._owner.clone()
        out = lifter.push(fr_d, t)
        x = torch.empty((2 * n, T, 17, 3), device="cuda")
        row_slot = torch.empty(n, dtype=torch.int32, device="cuda")
        _lib.check(lib.kasf_stream_track_front(ptr(fr_d), ptr(t.ids), ptr(t.slot), ptr(t.born), ptr(t.count), B, S_T, 0, R, T, ptr(ring), ptr(count), ptr(owner),
                                               ptr(lifter._width), ptr(lifter._height), ptr(lifter._r_tab), 1, ptr(x), ptr(row_slot), stream()))
        with torch.no_grad():
            pred = _forward_windows(lifter.model, x, n, 2, n)
        poses = torch.empty((n, 17, 3), device="cuda")
        valid, ids_out = torch.empty(n, dtype=torch.bool, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        frames_out = torch.empty(n, dtype=torch.int64, device="cuda")
        _lib.check(lib.kasf_stream_track_emit(ptr(pred), 1, ptr(count), ptr(owner), ptr(row_slot), n, T, ptr(lifter._fp_tab), 2, ptr(poses), ptr(valid),
                                              ptr(ids_out), ptr(frames_out), stream()))
        assert torch.equal(out.poses.view(n, 17, 3), poses) and torch.equal(out.valid.view(-1), valid), tick
        assert torch.equal(out.ids.view(-1), ids_out) and torch.equal(out.frames.view(-1), frames_out), tick
        assert torch.equal(lifter._ring, ring) and torch.equal(lifter._count, count) and torch.equal(lifter._owner, owner), tick
        assert valid.any() and out.poses.abs().sum() > 0


@pytest.mark.parametrize("name,params", [("demo", dict(min_hits=0)), ("default", dict())])
def test_behind_the_real_tracker(name, params):
    """Fixture box sequences -> SortTracker -> TrackedLifter.push against a loop that reads the TrackResult back and drives a plain StreamLifter: the poses are
    equal, fp32.  With the defaults (min_hits = 3) a track founded after the third tick is first emitted later, with born = 0: only the owner table starts
    its history."""
    import kasportsformer_amd as K
    z = np.load(os.path.join(GOLDEN, "track_sort.npz"), allow_pickle=False)
    dets, cnt = torch.from_numpy(z[f"{name}_dets"]).cuda(), torch.from_numpy(z[f"{name}_count"]).cuda()
    S, P, m = 32, 2, _model("fp32")
    trk = K.SortTracker(streams=1, slots=S, num_person=P, **params)
    lifter = K.TrackedLifter(m, 1280, 720, streams=1, track_slots=S, rows="persons", num_person=P)
    plain = K.StreamLifter(m, 1280, 720, slots=S)
    holder, pushed, starts, owner_only = {}, 0, 0, 0
    for tick in range(len(dets)):
        t = trk.update(dets[tick:tick + 1], cnt[tick:tick + 1])
        kp = torch.from_numpy(frames_for(tick, P, seed=11)).cuda()
        out = lifter.push(kp, t)
        c = int(t.count[0])
        ids, slot, born = t.ids[0].cpu().tolist(), t.slot[0].cpu().tolist(), t.born[0].cpu().tolist()
        for k in range(P):
            if k >= c:
                assert not out.valid[0, k] and not out.poses[0, k].any(), (tick, k)
                continue
            r = c - 1 - k
            if holder.get(slot[r]) != ids[r] or born[r]:
                plain.reset(slots=[slot[r]])
                holder[slot[r]] = ids[r]
                starts += 1
                owner_only += not born[r]
            want = plain.push(kp[k:k + 1], slots=[slot[r]])
            pushed += 1
            assert out.valid[0, k] and int(out.ids[0, k]) == ids[r] and int(out.frames[0, k]) == int(plain.counts[slot[r]]), (tick, k)
            assert torch.equal(out.poses[0, k], want[0]), (tick, k)
    assert pushed > 0 and starts > 0
    if "min_hits" not in params:
        assert owner_only > 0, "a history that only the owner table could start"


def test_coco_layout_and_push_heatmaps():
    """layout="coco" gives what push gives for the converted frames, push_heatmaps what push gives for the decoded ones, bit for bit."""
    import kasportsformer_amd as K
    from kasportsformer_amd.pose import convert_frames
    T, R = 27, 2
    n = B * R
    coco, plain = _lifter(layout="coco"), _lifter()
    hm_h36m, hm_coco, decoded = _lifter(), _lifter(layout="coco"), _lifter()
    g = torch.Generator().manual_seed(5)
    center = torch.tensor([[600.0, 350.0]] * n, device="cuda") + torch.arange(n, device="cuda")[:, None]
    scale = torch.tensor([[1.5, 2.0]] * n, device="cuda")
    for tick, arrays in enumerate(script(T, 8)[5:8]):
        t = _dev(arrays)
        kp = torch.from_numpy(frames_for(tick, n, seed=13)).cuda()
        keep = kp.clone()
        got, want = coco.push(kp, t), plain.push(convert_frames(kp), t)
        assert torch.equal(kp, keep)
        assert all(torch.equal(u, v) for u, v in zip(got, want)), tick
        hm = torch.rand((n, 17, 16, 12), generator=g).cuda()
        got = hm_h36m.push_heatmaps(hm, center, scale, t)
        got_coco = hm_coco.push_heatmaps(hm.view(B, R, 17, 16, 12), center.view(B, R, 2), scale.view(B, R, 2), t)
        want = decoded.push(K.heatmaps_to_keypoints(hm, center, scale, layout="h36m"), t)
        assert all(torch.equal(u, v) and torch.equal(w, v) for u, v, w in zip(got, want, got_coco)), tick
        assert want.valid.any() and want.poses.abs().sum() > 0


def test_a_tick_does_not_synchronise_with_the_host():
    import kasportsformer_amd as K
    z = np.load(os.path.join(GOLDEN, "track_sort.npz"), allow_pickle=False)
    dets, cnt = torch.from_numpy(z["demo_dets"]).cuda(), torch.from_numpy(z["demo_count"]).cuda()
    trk = K.SortTracker(streams=1, slots=32, min_hits=0, num_person=2)
    lifter = K.TrackedLifter(_model("fp32"), 1280, 720, streams=1, track_slots=32, rows="persons", num_person=2)
    kps = [torch.from_numpy(frames_for(tick, 2, seed=17)).cuda() for tick in range(3)]
    boxes, counts = [dets[i:i + 1].contiguous() for i in range(3)], [cnt[i:i + 1].contiguous() for i in range(3)]
    lifter.push(kps[0], trk.update(boxes[0], counts[0]))                      # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    raised, ok = False, False
    t = trk.update(boxes[1], counts[1])
    lifter.push(kps[1], t)
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:                                                                    # the control: the read-back a caller needed before
            t.ids.cpu()
        except RuntimeError:
            raised = True
        if raised:
            out = lifter.push(kps[2], trk.update(boxes[2], counts[2]))
            ok = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not raised:
        pytest.skip("this torch build does not raise on a device-to-host copy under set_sync_debug_mode('error'): the check would pass vacuously")
    assert ok and bool(out.valid.any())


def test_two_runs_give_the_same_bits():
    T, R = 27, 2
    runs = []
    for _ in range(2):
        run, xs = _FrontRun(T, "persons", R, True), []
        for tick, arrays in enumerate(script(T, 40)):
            x, row_slot = run.tick(arrays, torch.from_numpy(frames_for(tick, B * R, seed=19)).cuda())
            xs.append(x.clone())
        runs.append((xs, run.ring.clone()))
    assert all(torch.equal(u, v) for u, v in zip(runs[0][0], runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    (pa, ra), (pb, rb) = _poses(30), _poses(30)
    assert all(torch.equal(u, v) for u, v in zip(pa, pb)) and torch.equal(ra, rb)


def _poses(ticks):
    lifter, out = _lifter(), []
    for tick, arrays in enumerate(script(27, ticks)):
        out.append(lifter.push(torch.from_numpy(frames_for(tick, B * 2, seed=23)).cuda(), _dev(arrays)).poses.clone())
    return out, lifter._ring.clone()


def test_refusals_come_before_any_launch_and_reset_goes_with_the_tracker():
    import kasportsformer_amd as K
    lifter = _lifter()
    arrays = script(27, 8)
    kp = frames_for(0, 4)
    lifter.push(kp, _dev(arrays[6]))
    ring, count, owner = lifter._ring.clone(), lifter._count.clone(), lifter._owner.clone()
    t = _dev(arrays[7])
    bad = [(ValueError, lambda: lifter.push(kp[:3], t)), (ValueError, lambda: lifter.push(kp[:, :, :2], t)), (TypeError, lambda: lifter.push(kp.astype(np.float64), t)),
           (TypeError, lambda: lifter.push(kp.tolist(), t)), (RuntimeError, lambda: lifter.push(torch.zeros((4, 17, 3), device="meta"), t)),
           (RuntimeError, lambda: lifter.push(kp, SimpleNamespace(**{k: v.cpu() for k, v in vars(t).items()}))),
           (ValueError, lambda: lifter.push(kp, SimpleNamespace(**dict(vars(t), ids=t.ids[:, :3])))),
           (TypeError, lambda: lifter.push(kp, SimpleNamespace(**dict(vars(t), count=t.count.long())))),
           (TypeError, lambda: lifter.push(kp, None)), (TypeError, lambda: lifter.reset(streams=[0.5])), (ValueError, lambda: lifter.reset(streams=[2]))]
    for exc, call in bad:
        with pytest.raises(exc):
            call()
        assert torch.equal(lifter._ring, ring) and torch.equal(lifter._count, count) and torch.equal(lifter._owner, owner)
    for kw in (dict(lag=-1), dict(lag=27), dict(rows="people"), dict(layout="openpose"), dict(track_slots=65), dict(streams=3)):
        with pytest.raises(ValueError):
            _lifter(**kw)
    assert count.view(B, S_T)[0].any() and count.view(B, S_T)[1].any()
    lifter.reset(streams=[1])
    assert torch.equal(lifter._count.view(B, S_T)[0], count.view(B, S_T)[0]) and not lifter._count.view(B, S_T)[1].any() and not lifter._owner.view(B, S_T)[1].any()
    lifter.reset()
    assert not lifter._count.any() and not lifter._owner.any()
    out = lifter.push(kp, t)                                   # ids restart: every valid row begins a history
    assert out.frames[out.valid].tolist() == [1] * int(out.valid.sum()) and out.valid.any()
