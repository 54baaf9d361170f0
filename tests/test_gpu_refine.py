"""The recorded-track refinement on the GPU (kasportsformer_amd.refine_tracks, csrc/k_refine.hip): the cases of tests/test_refine_host_cpu.py through the public
function and the C entry on the device, equal to the fp32 restatement of include/kasf.h's rule (tests/refine_ref.py) bit for bit -- outputs and states --, the
same bits on a second run, a track alone against the track inside a batch, inputs unchanged, sentinels behind the outputs intact, the four forms recorded tracks
come in, host and device inputs.  A differing bit is a finding to explain, not a bar to loosen."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import ptr, stream
from tests.refine_ref import bundle, refine_np, weights
from tests.smooth_ref import SHAPES

pytestmark = pytest.mark.gpu
GAPS, RADII = (0, 1, 64), (0, 1, 32)
CAN = 9.0


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.uint32)


def sigma_of(radius):
    return 2.0 if radius < 32 else 11.0


@pytest.fixture(scope="module")
def bundles():
    """The inputs of every test here, made once: (J, C, score) -> (x, offsets)."""
    return {s: bundle(*s, seed=s[0]) for s in SHAPES}


@pytest.mark.parametrize("J,Cn,score", SHAPES)
def test_refine_tracks_equals_the_restatement_bit_for_bit(bundles, J, Cn, score):
    import kasportsformer_amd as K
    x, off = bundles[(J, Cn, score)]
    xd = torch.from_numpy(x).cuda()
    seen = set()
    for max_gap in GAPS:
        for radius in RADII:
            w, _ = weights(sigma_of(radius), radius)
            want, want_state = refine_np(x, off, score, 0.3, max_gap, w, radius)
            out, state = K.refine_tracks(xd, offsets=off, score=score, min_score=0.3, max_gap=max_gap, sigma=sigma_of(radius), radius=radius, return_state=True)
            assert out.shape == xd.shape and out.dtype == torch.float32 and state.shape == xd.shape[:2] and state.dtype == torch.uint8 and state.is_cuda
            assert np.array_equal(state.cpu().numpy(), want_state), (max_gap, radius, np.argwhere(state.cpu().numpy() != want_state)[:4])
            diff = np.argwhere(bits(out) != bits(want))
            assert diff.size == 0, (max_gap, radius, diff[:8])
            again = K.refine_tracks(xd, offsets=off, score=score, min_score=0.3, max_gap=max_gap, sigma=sigma_of(radius), radius=radius)
            assert np.array_equal(bits(again), bits(out))          # the same bits on a second run, and without a state output
            seen |= set(np.unique(want_state).tolist())
    assert seen == {0, 1, 2, 3} and np.array_equal(bits(xd), bits(x))


@pytest.mark.parametrize("J,Cn,score", SHAPES[:2])
def test_a_track_alone_equals_the_track_in_the_batch(bundles, J, Cn, score):
    import kasportsformer_amd as K
    x, off = bundles[(J, Cn, score)]
    out, state = K.refine_tracks(x, offsets=off, score=score, return_state=True)
    for p in (0, 7, len(off) - 2):
        lo, hi = int(off[p]), int(off[p + 1])
        if hi > lo:
            o1, s1 = K.refine_tracks(x[lo:hi], score=score, return_state=True)
            assert np.array_equal(bits(o1), bits(out[lo:hi])) and torch.equal(s1, state[lo:hi])


@pytest.mark.parametrize("offsets", ["exact", "clamped", "inner"])
def test_the_entry_clamps_offsets_and_writes_nothing_else(offsets):
    """The C entry with sentinels around out and state: offsets beyond [0, N] are clamped, rows of no track are not written, x is only read."""
    from kasportsformer_amd import _lib
    J, Cn, score = SHAPES[0]
    x, off = bundle(J, Cn, score, seed=3, offsets=offsets)
    N, P = x.shape[0], len(off) - 1
    w, radius = weights(2.0)
    want, want_state = refine_np(x, off, score, 0.3, 15, w, radius)
    none = want_state[:, 0] == 255
    want[none], want_state[none] = CAN, 77
    assert none.sum() == (5 if offsets == "inner" else 0)
    xd, od = torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda()
    out_buf = torch.full((x.size + 128,), CAN, device="cuda")
    state_buf = torch.full((N * J + 128,), 77, dtype=torch.uint8, device="cuda")
    out, state = out_buf[64:64 + x.size].view(x.shape), state_buf[64:64 + N * J].view(N, J)
    q = _lib.KasfRefineParams(0.3, 15, radius, (C.c_float * 33)(*w.tolist()))
    _lib.check(_lib.load().kasf_tracks_refine(ptr(xd), ptr(od), N, P, J, Cn, int(score), C.byref(q), ptr(out), ptr(state), stream()))
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(state.cpu().numpy(), want_state)
    assert (out_buf[:64] == CAN).all() and (out_buf[-64:] == CAN).all() and (state_buf[:64] == 77).all() and (state_buf[-64:] == 77).all()
    assert np.array_equal(bits(xd), bits(x)) and np.array_equal(od.cpu().numpy(), off)
    out2 = torch.full_like(out, CAN)
    _lib.check(_lib.load().kasf_tracks_refine(ptr(xd), ptr(od), N, P, J, Cn, int(score), C.byref(q), ptr(out2), None, stream()))      # state = NULL
    assert np.array_equal(bits(out2), bits(want))


def test_more_tiles_than_the_grid_has_workgroups():
    """65,536 tiles of 64 frames and 3,000 frames more, one joint of one channel (16 MB): the frames past the grid's 65,536 workgroups are a second pass of the
    kernel's tile loop.  Tracks of 1,000 frames; those of the second pass, and one that straddles it, equal the same tracks alone."""
    import kasportsformer_amd as K
    n, P = 1000, (65536 * 64 + 3000) // 1000
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((P * n, 1, 1), device="cuda", generator=g) * 1000.0
    x[::7] = float("nan")
    x[P * n - 2500:P * n - 2480] = float("nan")                    # a gap longer than max_gap, in the second pass
    off = np.arange(P + 1, dtype=np.int64) * n
    out, state = K.refine_tracks(x, offsets=off, score=False, return_state=True)
    first_of_second_pass = 65536 * 64 // n                          # this track straddles the last tile of the first pass
    for p in (0, first_of_second_pass, P - 3, P - 1):
        o1, s1 = K.refine_tracks(x[p * n:(p + 1) * n], score=False, return_state=True)
        assert np.array_equal(bits(o1), bits(out[p * n:(p + 1) * n])) and torch.equal(s1, state[p * n:(p + 1) * n]), p
    tail = state[65536 * 64:]
    assert (tail == 1).any() and (tail == 3).any() and (tail == 0).any() and not torch.isnan(out[65536 * 64:][tail != 3]).any()


@pytest.mark.parametrize("J,Cn,score", SHAPES[:2])
def test_the_four_forms_from_the_host_and_from_the_device(bundles, J, Cn, score):
    import kasportsformer_amd as K
    x, off = bundles[(J, Cn, score)]
    w, radius = weights(2.0)
    want, want_state = refine_np(x, off, score, 0.3, 15, w, radius)
    xd = torch.from_numpy(x).cuda()
    packed, st = K.refine_tracks(xd, offsets=off, score=score, return_state=True)
    assert np.array_equal(bits(packed), bits(want)) and np.array_equal(st.cpu().numpy(), want_state)
    host, st_h = K.refine_tracks(x, offsets=torch.from_numpy(off), score=score, return_state=True)             # from the host
    assert host.is_cuda and np.array_equal(bits(host), bits(packed)) and torch.equal(st_h, st)
    pieces = [x[a:b] for a, b in zip(off[:-1], off[1:])]
    parts, states = K.refine_tracks(pieces, score=score, return_state=True)                                    # a list -> lists
    assert [len(p) for p in parts] == [len(p) for p in pieces] == [len(s) for s in states]
    assert np.array_equal(bits(torch.cat(parts)), bits(want)) and np.array_equal(torch.cat(states).cpu().numpy(), want_state)
    mixed = K.refine_tracks([torch.from_numpy(p).cuda() if i % 2 else p for i, p in enumerate(pieces)], score=score)
    assert np.array_equal(bits(torch.cat(mixed)), bits(want))
    a, b = int(off[-2]), int(off[-1])
    one, s_one = K.refine_tracks(xd[a:b], score=score, return_state=True)                                      # [N,J,Ct]: one track
    assert one.shape == xd[a:b].shape and s_one.shape == (b - a, J) and np.array_equal(bits(one), bits(want[a:b]))
    two, s_two = K.refine_tracks(np.stack([x[a:b], x[:b - a]]), score=score, return_state=True)                # [P,N,J,Ct]
    assert two.shape == (2, b - a, J, x.shape[2]) and s_two.shape == (2, b - a, J)
    assert np.array_equal(bits(two[0]), bits(want[a:b])) and torch.equal(s_two[0], s_one)
    assert np.array_equal(bits(two[1]), bits(refine_np(np.ascontiguousarray(x[:b - a]), [0, b - a], score, 0.3, 15, w, radius)[0]))
    assert K.refine_tracks([], score=score) == [] and K.refine_tracks([], score=score, return_state=True) == ([], [])
    empty = K.refine_tracks(x[:0], score=score)
    assert empty.shape == (0, J, x.shape[2]) and empty.is_cuda
    fill = K.refine_tracks(xd, offsets=off, score=score, sigma=None)                                           # the gap fill alone
    assert np.array_equal(bits(fill), bits(refine_np(x, off, score, 0.3, 15, None, 0)[0]))
    assert np.array_equal(bits(xd), bits(x))
