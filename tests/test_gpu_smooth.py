"""The One-Euro filter on the GPU (kasportsformer_amd.OneEuroFilter / smooth_tracks, csrc/k_smooth.hip): the cases of tests/test_smooth_host_cpu.py through the
public classes on the device, equal to the fp32 restatement of include/kasf.h's rule (tests/smooth_ref.py) bit for bit -- outputs and state --, the same bits on
a second run, a row alone against the row inside a batch, inputs and TrackResult unchanged, and a TrackedLifter tick that a filter never pushed to leaves as it
was.  A differing bit is a finding to explain, not a bar to loosen."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.gpu_util import make_pair, ptr, stream
from tests.smooth_ref import SHAPES, new_state, params, push_np, rows_for, tracked_np, tracks_np
from tests.tracked_ref import Cases, frames_for, script

pytestmark = pytest.mark.gpu
B, S_T, T = 2, 4, 5
KW = dict(rate=30.0, min_cutoff=1.0, beta=0.01, d_cutoff=1.0, min_score=0.3, max_hold=2)
P_REF = params(**KW)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def _dev(arrays):
    return SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()})


def _state_equals(f, state):
    return (np.array_equal(bits(f._xhat), bits(state["xhat"])) and np.array_equal(bits(f._dxhat), bits(state["dxhat"]))
            and np.array_equal(f._last.cpu().numpy(), state["last"]) and (f._owner is None or np.array_equal(f._owner.cpu().numpy(), state["owner"])))


@pytest.mark.parametrize("J,Cn,score", SHAPES)
@pytest.mark.parametrize("rows,R", [("persons", 2), ("tracks", 4)])
def test_tracked_filter_equals_the_restatement_bit_for_bit(rows, R, J, Cn, score):
    import kasportsformer_amd as K
    n = B * R
    state, cases = new_state(B * S_T, J, Cn), Cases(T, S_T, R)
    ticks, want, tick = [], [], 0
    for i, arrays in enumerate(script(T, 3 * T + 4)):
        x = rows_for(i, n, J, Cn, score, seed=T)
        step = 3 if i == 8 else 1                                  # one push comes after two dropped frames
        tick += step - 1
        owner_before = state["owner"].copy()
        out, row_slot, reset, why = tracked_np(state, P_REF, x, arrays, rows, R, tick, score)
        cases.see(i, arrays, owner_before, state["owner"], state["count"], row_slot, reset, why)
        tick += 1
        ticks.append((x, arrays, step))
        want.append(out)
    assert not cases.missing(), cases.missing()
    runs = []
    for _ in range(2):
        f = K.OneEuroFilter(streams=B, track_slots=S_T, rows=rows, num_person=2, joints=J, channels=Cn, score=score, **KW)
        got = []
        for i, (x, arrays, step) in enumerate(ticks):
            xd, t = torch.from_numpy(x).cuda(), _dev(arrays)
            xd = xd.view(B, R, J, -1) if i % 2 else xd             # both shapes push takes
            keep = [xd.clone()] + [getattr(t, k).clone() for k in ("ids", "slot", "born", "count")]
            out = f.push(xd, t, ticks=step)
            assert out.shape == xd.shape and out.is_cuda and out.dtype == torch.float32
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(keep, [xd, t.ids, t.slot, t.born, t.count])), i
            got.append(out.view(n, J, -1))
        assert f.tick == tick and _state_equals(f, state)
        runs.append(torch.stack(got))
    diff = np.argwhere(bits(runs[0]) != bits(np.stack(want)))
    assert diff.size == 0, diff[:8]
    assert np.array_equal(bits(runs[0]), bits(runs[1]))            # the same bits on a second run
    f.reset(streams=[1])
    assert (f._last.view(B, S_T, J)[1] == -1).all() and (f._owner.view(B, S_T)[1] == 0).all()
    assert np.array_equal(f._last.view(B, S_T, J)[0].cpu().numpy(), state["last"].reshape(B, S_T, J)[0])
    f.reset()
    assert (f._last == -1).all() and (f._owner == 0).all()


@pytest.mark.parametrize("J,Cn,score", SHAPES)
def test_slot_filter_equals_the_restatement_and_a_row_alone_equals_the_row_in_a_batch(J, Cn, score):
    import kasportsformer_amd as K
    S = 5
    state, alone_state = new_state(S, J, Cn), new_state(S, J, Cn)
    f, alone = (K.OneEuroFilter(slots=S, joints=J, channels=Cn, score=score, **KW) for _ in range(2))
    tick = 0
    for i in range(14):
        slots = (None, [3, 0], np.array([1, 4, 3]))[i % 3]
        K_rows = S if slots is None else len(slots)
        x = rows_for(i, K_rows, J, Cn, score, seed=3)
        step = 3 if i == 9 else 1
        tick += step - 1
        want = push_np(state, P_REF, x, slots, tick, score)
        tick += 1
        xd = torch.from_numpy(x).cuda() if i % 2 else x            # a host array is uploaded, a device tensor read in place
        out = f.push(xd, slots=slots, ticks=step)
        assert np.array_equal(bits(out), bits(want)), (i, np.argwhere(bits(out) != bits(want))[:8])
        if i % 2:
            assert np.array_equal(bits(xd), bits(x))
        r = 3 if slots is None else list(slots).index(3)           # slot 3 is in every call: alone, it gives the same bits
        one = alone.push(x[r:r + 1], slots=[3], ticks=step)
        assert np.array_equal(bits(one[0]), bits(want[r])), i
    assert f.tick == tick == alone.tick and _state_equals(f, state)
    assert np.array_equal(bits(alone._xhat[3]), bits(state["xhat"][3])) and (alone._last[[0, 1, 2, 4]] == -1).all()
    assert f.push(np.zeros((0, J, Cn + int(score)), np.float32), slots=[]).shape == (0, J, Cn + int(score)) and f.tick == tick + 1
    f.reset(slots=[3])
    assert (f._last[3] == -1).all() and np.array_equal(f._last[4].cpu().numpy(), state["last"][4])
    with pytest.raises(ValueError):                                # refused before any launch: state and tick as they were
        f.push(np.zeros((2, J, Cn + int(score)), np.float32), slots=[0, S])
    assert f.tick == tick + 1 and np.array_equal(f._last[4].cpu().numpy(), state["last"][4])


def test_entry_copies_a_row_with_an_id_outside_the_slots_through():
    """What the Python surface refuses: ids outside [0, S) reach the entry point itself, with canaries around the state."""
    from kasportsformer_amd import _lib
    S, J, Cn, score, CAN = 5, 17, 2, True, 12345.5
    state = new_state(S, J, Cn, fill=-7.0)
    bufs = {k: torch.full((S * J * Cn + 128,), CAN, device="cuda") for k in ("xhat", "dxhat")}
    xhat, dxhat = (bufs[k][64:64 + S * J * Cn].view(S, J, Cn) for k in ("xhat", "dxhat"))
    xhat.fill_(-7.0), dxhat.fill_(-7.0)
    last_buf = torch.full((S * J + 128,), 0x5A5A, dtype=torch.int64, device="cuda")
    last = last_buf[64:64 + S * J].view(S, J)
    last.fill_(-1)
    q = _lib.KasfOneEuroParams(float(P_REF["dt"]), 1.0, 1.0, 0.01, 0.3, 2)
    slots = np.array([1, S, 4, -1], np.int32)
    for tick in range(4):
        x = rows_for(tick, 4, J, Cn, score, seed=4)
        want = push_np(state, P_REF, x, slots, tick, score)
        xd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(slots).cuda()
        out_buf = torch.full((x.size + 128,), CAN, device="cuda")
        out = out_buf[64:64 + x.size].view(x.shape)
        _lib.check(_lib.load().kasf_one_euro_push(ptr(xd), ptr(sd), 4, S, J, Cn, 1, C.byref(q), tick, ptr(xhat), ptr(dxhat), ptr(last), ptr(out), stream()))
        assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(out[[1, 3]]), bits(x[[1, 3]]))
        assert (out_buf[:64] == CAN).all() and (out_buf[-64:] == CAN).all()
    assert np.array_equal(bits(xhat), bits(state["xhat"])) and np.array_equal(bits(dxhat), bits(state["dxhat"])) and np.array_equal(last.cpu().numpy(), state["last"])
    assert all((b[:64] == CAN).all() and (b[-64:] == CAN).all() for b in bufs.values()) and (last_buf[:64] == 0x5A5A).all() and (last_buf[-64:] == 0x5A5A).all()


def test_more_rows_than_the_grid_has_workgroups():
    """65,539 slots of one joint: the rows past the grid's 65,536 workgroups are a second pass of the kernel's row loop."""
    import kasportsformer_amd as K
    S = 65536 + 3
    g = np.random.default_rng(8)
    x = (g.random((3, S, 1)) * 1000.0).astype(np.float32)
    x[1, ::7] = np.nan
    f = K.OneEuroFilter(slots=S, joints=1, channels=1, score=False, **KW)
    got = torch.stack([f.push(torch.from_numpy(x[i]).cuda().view(S, 1, 1)) for i in range(3)])
    want = tracks_np(P_REF, x, [0, 3], False)                     # the same three frames as one track of S joints
    assert np.array_equal(bits(got.view(3, S, 1)), bits(want))


@pytest.mark.parametrize("J,Cn,score", SHAPES)
def test_smooth_tracks_equals_the_restatement_and_push_frame_by_frame(J, Cn, score):
    import kasportsformer_amd as K
    lengths = [0, 1, 2, 40]
    off = np.cumsum([0] + lengths).astype(np.int64)
    x = np.concatenate([rows_for(100 + f, 1, J, Cn, score, seed=9) for f in range(off[-1])])
    want = tracks_np(P_REF, x, off, score)
    xd = torch.from_numpy(x).cuda()
    packed = K.smooth_tracks(xd, offsets=off, score=score, **KW)
    assert np.array_equal(bits(packed), bits(want)) and np.array_equal(bits(xd), bits(x))
    assert np.array_equal(bits(K.smooth_tracks(x, offsets=torch.from_numpy(off), score=score, **KW)), bits(packed))      # from the host; a second run
    parts = K.smooth_tracks([x[a:b] for a, b in zip(off[:-1], off[1:])], score=score, **KW)
    assert [len(p) for p in parts] == lengths and np.array_equal(bits(torch.cat(parts)), bits(want))
    one = K.smooth_tracks(xd[3:], score=score, **KW)               # [N,J,Ct]: one track
    assert one.shape == xd[3:].shape and np.array_equal(bits(one), bits(want[3:]))
    two = K.smooth_tracks(np.stack([x[3:], x[3:][::-1]]), score=score, **KW)      # [P,N,J,Ct]
    assert two.shape == (2, 40, J, x.shape[2]) and np.array_equal(bits(two[0]), bits(want[3:]))
    assert np.array_equal(bits(two[1]), bits(tracks_np(P_REF, np.ascontiguousarray(x[3:][::-1]), [0, 40], score)))
    f = K.OneEuroFilter(slots=1, joints=J, channels=Cn, score=score, **KW)
    live = torch.cat([f.push(xd[3 + i:4 + i]) for i in range(40)])
    assert np.array_equal(bits(live), bits(one))                   # the recorded form is push frame by frame


def test_a_filter_never_pushed_to_leaves_the_tracked_lifter_tick_as_it_was():
    import kasportsformer_amd as K
    model = make_pair(1, 27, "fp32")[1].eval()
    ticks = [(torch.from_numpy(frames_for(i, B * 2, seed=1)).cuda(), _dev(arrays)) for i, arrays in enumerate(script(27, 4))]

    def run():
        lifter = K.TrackedLifter(model, [1280, 1437], [720, 913], streams=B, track_slots=S_T, rows="persons", num_person=2)
        return [lifter.push(kp, t) for kp, t in ticks]
    before = run()
    filters = [K.OneEuroFilter(streams=B, track_slots=S_T, rows="persons", num_person=2),
               K.OneEuroFilter(streams=B, track_slots=S_T, rows="persons", num_person=2, channels=3, score=False), K.OneEuroFilter(slots=4)]
    after = run()
    for a, b in zip(before, after):
        assert np.array_equal(bits(a.poses), bits(b.poses)) and torch.equal(a.valid, b.valid) and torch.equal(a.ids, b.ids) and torch.equal(a.frames, b.frames)
    # ... and with the two filters in the tick, the lifter gets the filtered keypoints and the rows agree on their slots
    lifter = K.TrackedLifter(model, [1280, 1437], [720, 913], streams=B, track_slots=S_T, rows="persons", num_person=2)
    plain = K.TrackedLifter(model, [1280, 1437], [720, 913], streams=B, track_slots=S_T, rows="persons", num_person=2)
    for kp, t in ticks:
        kf = filters[0].push(kp, t)
        out = lifter.push(kf, t)
        poses = filters[1].push(out.poses, t)
        assert poses.shape == out.poses.shape and np.array_equal(bits(out.poses), bits(plain.push(kf, t).poses))
        assert np.array_equal(bits(poses[~out.valid]), bits(out.poses[~out.valid]))
    assert np.array_equal(filters[0]._owner.cpu().numpy(), lifter._owner.cpu().numpy()) and all(f.tick == 4 for f in filters[:2]) and filters[2].tick == 0
