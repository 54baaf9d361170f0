"""Constant limb lengths on the GPU (kasportsformer_amd.bone_lengths / fix_bone_lengths / BoneLengthFilter, csrc/k_bones.hip): the cases of
tests/test_bones_host_cpu.py through the public calls on the device, equal to the fp32 restatement of include/kasf.h's rule (tests/bones_ref.py) bit for bit --
medians, counts, walked frames, live state --, the same bits on a second run, a track alone against the track inside a batch, the four input forms, rows behind N
untouched, inputs and TrackResult unchanged, and lift_track followed by fix_bone_lengths on the small golden model.  The device's square root and divide being
correctly rounded is what the equality rests on; a differing bit is a finding to explain, not a bar to loosen."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bones_ref as R
from tests.gpu_util import make_pair, ptr, stream
from tests.tracked_ref import Cases, script

pytestmark = pytest.mark.gpu
B, S_T, T = 2, 4, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def same(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def tracks():
    x, off = R.median_tracks()
    L, n = R.median_np(x, off)
    return SimpleNamespace(x=x, off=off, L=L, n=n)


def test_medians_equal_the_restatement_bit_for_bit(tracks):
    import kasportsformer_amd as K
    xd = torch.from_numpy(tracks.x).cuda()
    keep = xd.clone()
    L, n = K.bone_lengths(xd, tracks.off)
    assert L.is_cuda and L.dtype == torch.float32 and n.dtype == torch.int32 and tuple(L.shape) == tuple(n.shape) == tracks.L.shape
    diff = np.argwhere(bits(L) != bits(tracks.L))
    assert diff.size == 0, (diff[:8], L.cpu().numpy()[tuple(diff[0])], tracks.L[tuple(diff[0])])
    assert np.array_equal(n.cpu().numpy(), tracks.n) and same(xd, keep)
    L2, n2 = K.bone_lengths(xd, tracks.off)                          # the same bits on a second run
    assert same(L, L2) and torch.equal(n, n2)
    for p in (4, 7, 11):                                           # a track alone against the track inside the batch
        a, b = int(tracks.off[p]), int(tracks.off[p + 1])
        La, na = K.bone_lengths(tracks.x[a:b])
        assert same(La[0], tracks.L[p]) and np.array_equal(na[0].cpu().numpy(), tracks.n[p])


def test_medians_over_sixty_binades_with_and_without_counts():
    """Lengths that survive the square and its root exactly, powers of two from 2^-60 to 2^59, so the select sees every exponent byte; counts NULL and not."""
    from kasportsformer_amd import _lib
    _, off = R.select_scratch()
    P, N = len(off) - 1, int(off[-1])
    e = np.random.default_rng(3).integers(-60, 60, (N, 16))
    x = np.zeros((N, 17, 3), np.float32)
    for k in range(16):
        x[:, k + 1] = x[:, R.PARENTS[k]]
        x[:, k + 1, k % 3] += np.ldexp(np.float32(1), e[:, k]).astype(np.float32)
    x[::11, 3] = x[::11, 2]                                        # and a bone of length 0 now and then
    xd, offd = torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda()
    want_L, want_n = R.median_np(x, off)
    assert len(np.unique(want_L)) > 20
    scratch, L, n = torch.empty(16 * N, device="cuda"), torch.empty((P, 16), device="cuda"), torch.empty((P, 16), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().kasf_bone_median(ptr(xd), ptr(offd), N, P, ptr(scratch), ptr(L), ptr(n), stream()))
    assert same(L, want_L) and np.array_equal(n.cpu().numpy(), want_n)
    L.fill_(7.0)
    _lib.check(_lib.load().kasf_bone_median(ptr(xd), ptr(offd), N, P, ptr(scratch), ptr(L), None, stream()))
    assert same(L, want_L) and np.array_equal(n.cpu().numpy(), want_n)


@pytest.mark.parametrize("symmetric", [False, True])
def test_fix_equals_the_restatement_in_all_four_forms(tracks, symmetric):
    import kasportsformer_amd as K
    x, off = tracks.x, tracks.off
    want = R.apply_np(x, off, tracks.L, symmetric)
    xd = torch.from_numpy(x).cuda()
    keep = xd.clone()
    got, table = K.fix_bone_lengths(xd, off, symmetric=symmetric, return_lengths=True)
    diff = np.argwhere(bits(got) != bits(want))
    assert diff.size == 0, diff[:8]
    assert same(table, tracks.L) and same(xd, keep) and got.is_cuda and got.shape == xd.shape
    assert same(K.fix_bone_lengths(xd, off, symmetric=symmetric), got)                                   # the same bits on a second run
    bad = ~R.frames_usable(x)
    assert bad.any() and same(got[torch.from_numpy(bad).cuda()], x[bad])
    parts = [x[a:b] for a, b in zip(off[:-1], off[1:])]
    as_list = K.fix_bone_lengths([torch.from_numpy(p).cuda() if i % 2 else p for i, p in enumerate(parts)], symmetric=symmetric)
    assert len(as_list) == len(parts) and all(same(a, want[s:e]) for a, s, e in zip(as_list, off[:-1], off[1:]))
    for p in (4, 7, 11):                                           # one track [N,17,3]: alone against inside the batch
        a, b = int(off[p]), int(off[p + 1])
        assert same(K.fix_bone_lengths(x[a:b], symmetric=symmetric), want[a:b])
    cube = np.stack([parts[5], parts[6][:64], parts[7][100:164]])  # [P,N,17,3]
    want_cube = np.stack([R.fix_np(c, np.array([0, 64]), symmetric) for c in cube])
    got_cube = K.fix_bone_lengths(cube, symmetric=symmetric)
    assert tuple(got_cube.shape) == cube.shape and same(got_cube, want_cube)


@pytest.mark.parametrize("symmetric", [False, True])
def test_given_tables_shared_and_per_track(tracks, symmetric):
    import kasportsformer_amd as K
    x, off = tracks.x, tracks.off
    one, none = tracks.L.copy(), tracks.L.copy()
    one[:, 3], one[1::2, 10] = 0, 0                                # one partner 0
    none[:, [1, 4, 7, 15]] = 0                                     # L = 0: the bone is left alone
    for tab in (one, none, np.ascontiguousarray(tracks.L[7])):
        got = K.fix_bone_lengths(x, off, lengths=torch.from_numpy(tab).cuda() if tab.ndim == 1 else tab, symmetric=symmetric)
        want = R.apply_np(x, off, tab, symmetric)
        diff = np.argwhere(bits(got) != bits(want))
        assert diff.size == 0, diff[:8]
    # and the walk holds the fp64 bound of tests/test_bones_cpu.py on what it scaled
    L = R.symmetric_np(tracks.L[7]) if symmetric else tracks.L[7]
    a, b = int(off[7]), int(off[8])
    y = K.fix_bone_lengths(x[a:b], lengths=tracks.L[7], symmetric=symmetric).cpu().numpy()
    assert R.length_excess(y, L.astype(np.float64), np.ones((b - a, 16), bool)) <= 0


def test_rows_behind_n_are_untouched_and_unaligned_arrays_work(tracks):
    from kasportsformer_amd import _lib
    lib = _lib.load()
    N, extra = 300, 5
    x = tracks.x[int(tracks.off[7]):int(tracks.off[8])]
    off = np.array([0, 100, 300], np.int64)
    L, n = R.median_np(x, off)
    want = R.apply_np(x, off, L, False)
    for shift in (0, 1):                                           # shift 1: no 16-byte alignment, the scalar tile loads
        buf = torch.zeros((N + extra) * 51 + 4, device="cuda")
        obuf = torch.full(((N + extra) * 51 + 4,), 9.0, device="cuda")
        xin, out = buf[shift:shift + (N + extra) * 51].view(-1, 17, 3), obuf[shift:shift + (N + extra) * 51].view(-1, 17, 3)
        xin[:N] = torch.from_numpy(x).cuda()
        xin[N:] = 3.0
        scratch, Ld = torch.full((16 * N + 8,), 9.0, device="cuda"), torch.full((3, 16), 9.0, device="cuda")
        nd, offd = torch.full((3, 16), -7, dtype=torch.int32, device="cuda"), torch.from_numpy(off).cuda()
        _lib.check(lib.kasf_bone_median(xin.data_ptr(), ptr(offd), N, 2, ptr(scratch), ptr(Ld), ptr(nd), stream()))
        _lib.check(lib.kasf_bone_apply(xin.data_ptr(), ptr(offd), N, 2, ptr(Ld), 1, 0, out.data_ptr(), stream()))
        assert same(Ld[:2], L) and np.array_equal(nd[:2].cpu().numpy(), n) and (Ld[2] == 9.0).all() and (nd[2] == -7).all() and (scratch[16 * N:] == 9.0).all()
        assert same(out[:N], want) and (out[N:] == 9.0).all() and (obuf[:shift] == 9.0).all() and (obuf[shift + (N + extra) * 51:] == 9.0).all()
        assert same(xin[:N], x) and (xin[N:] == 3.0).all()


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("window", [1, 2, 5])
def test_slot_filter_equals_the_restatement_and_a_row_alone_equals_the_row_in_a_batch(window, symmetric):
    import kasportsformer_amd as K
    S = 5
    runs = []
    for run in range(2):
        f, st = K.BoneLengthFilter(slots=S, window=window, symmetric=symmetric), R.new_state(S)
        solo, got, want = K.BoneLengthFilter(slots=S, window=window, symmetric=symmetric), [], []
        for i in range(14):
            slots = (None, [3, 0], [4, 1])[i % 3]
            K_ = S if slots is None else len(slots)
            x = R.live_rows(i, K_, seed=3)
            xd = torch.from_numpy(x).cuda() if i % 2 else x
            want.append(R.push_np(st, x, slots, window, symmetric))
            out = f.push(xd, slots=slots)
            assert out.is_cuda and tuple(out.shape) == x.shape and same(xd, x)
            got.append(out)
            for r, g in enumerate(range(S) if slots is None else slots):                                 # each row alone, in a filter of its own
                assert same(solo.push(x[r:r + 1], slots=[g]), out[r:r + 1]), (i, r)
            live = st["cnt"] > 0
            assert np.array_equal(f._cnt.cpu().numpy(), st["cnt"]) and np.array_equal(bits(f._len)[live], bits(st["len"])[live]), i
        for a, b in zip(got, want):
            assert same(a, b), np.argwhere(bits(a) != bits(b))[:8]
        runs.append(torch.cat(got))
    assert same(runs[0], runs[1])                                   # the same bits on a second run
    f.reset(slots=[2])
    assert (f._cnt[2] == 0).all() and np.array_equal(f._cnt[3].cpu().numpy(), st["cnt"][3])
    f.reset()
    assert (f._cnt == 0).all()


def _dev(arrays):
    return SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in arrays.items()})


@pytest.mark.parametrize("rows,R_", [("persons", 2), ("tracks", 4)])
def test_tracked_filter_equals_the_restatement_and_agrees_with_the_one_euro_filter(rows, R_):
    import kasportsformer_amd as K
    n, window = B * R_, 3
    state, cases = R.new_state(B * S_T), Cases(T, S_T, R_)
    f = K.BoneLengthFilter(streams=B, track_slots=S_T, rows=rows, num_person=2, window=window, symmetric=True)
    euro = K.OneEuroFilter(streams=B, track_slots=S_T, rows=rows, num_person=2, joints=17, channels=3, score=False)
    for i, arrays in enumerate(script(T, 3 * T + 4)):
        x = R.live_rows(i, n, seed=T)
        owner_before = state["owner"].copy()
        want, row_slot, reset, why = R.tracked_np(state, x, arrays, rows, R_, window, True)
        cases.see(i, arrays, owner_before, state["owner"], state["count"], row_slot, reset, why)
        xd, t = torch.from_numpy(x).cuda(), _dev(arrays)
        xd = xd.view(B, R_, 17, 3) if i % 2 else xd
        keep = [xd.clone()] + [getattr(t, k).clone() for k in ("ids", "slot", "born", "count")]
        out = f.push(xd, t)
        euro.push(xd, t)
        assert out.shape == xd.shape and same(out.view(n, 17, 3), want), (i, np.argwhere(bits(out.view(n, 17, 3)) != bits(want))[:8])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(keep, [xd, t.ids, t.slot, t.born, t.count])), i
        live = state["cnt"] > 0
        assert np.array_equal(f._cnt.cpu().numpy(), state["cnt"]) and np.array_equal(bits(f._len)[live], bits(state["len"])[live]), i
        assert np.array_equal(f._owner.cpu().numpy(), state["owner"]) and torch.equal(f._owner, euro._owner), i
    assert not cases.missing(), cases.missing()
    f.reset(streams=[1])
    assert (f._cnt.view(B, S_T, 16)[1] == 0).all() and (f._owner.view(B, S_T)[1] == 0).all()
    assert np.array_equal(f._cnt.view(B, S_T, 16)[0].cpu().numpy(), state["cnt"].reshape(B, S_T, 16)[0])


def test_lift_then_fix_gives_constant_bones_on_the_golden_model():
    import kasportsformer_amd as K
    fx = np.load(os.path.join(GOLDEN, "lift_e2e.npz"))
    model = make_pair(2, 27, "fp32")[1].eval()
    poses = K.lift_track(model, fx["track_n61"], int(fx["width"]), int(fx["height"]))
    fixed, table = K.fix_bone_lengths(poses, return_lengths=True)
    assert fixed.shape == poses.shape and fixed.is_cuda
    cube, y = poses.cpu().numpy().reshape(-1, 61, 17, 3), fixed.cpu().numpy().reshape(-1, 61, 17, 3)
    L = table.cpu().numpy().astype(np.float64)
    assert np.isfinite(y).all() and L.shape == (len(cube), 16) and (L > 0).all()
    assert same(y, np.stack([R.fix_np(c, np.array([0, 61])) for c in cube]))
    for p in range(len(y)):
        assert R.length_excess(y[p], L[p], np.ones((61, 16), bool)) <= 0
    assert same(y[:, :, 0], cube[:, :, 0])                          # the root stays where it was
