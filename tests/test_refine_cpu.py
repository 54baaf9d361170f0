"""The rule of include/kasf.h's kasf_tracks_refine, checked on its numpy restatement alone (tests/refine_ref.py): the properties the header claims for it, the
state codes on a hand-written mask, fp32 against the same statements in fp64, and a sanity check of what the rule does to a synthetic track next to the causal
filter it stands beside.  The kernel is held to this restatement bit for bit in tests/test_refine_host_cpu.py (its source, on the host) and
tests/test_gpu_refine.py (on the device)."""
import numpy as np
import pytest

from tests import smooth_ref
from tests.refine_ref import HELD, INTERPOLATED, LEFT, USABLE, refine_np, same_bits, synthetic_track, weights

W, RADIUS = weights(2.0)                    # the defaults: sigma 2 frames, radius 6
MAX_GAP = 4


def keypoints(n, J=3, value=None, seed=0):
    """[n, J, 3] fp32 keypoints, every joint usable: `value`, or noise around 300 px."""
    rng = np.random.default_rng(seed)
    x = np.empty((n, J, 3), np.float32)
    x[..., :2] = value if value is not None else rng.normal(300.0, 40.0, (n, J, 2))
    x[..., 2] = 0.9
    return x


def mask_track(mask):
    """One joint from a string: 'u' a usable frame, '.' a gated one (score 0.1, a wild position)."""
    x = keypoints(len(mask), J=1, seed=len(mask))
    for f, ch in enumerate(mask):
        if ch == ".":
            x[f, 0] = (5000.0, -5000.0, 0.1)
    return x


def states(mask, max_gap=MAX_GAP):
    x = mask_track(mask)
    return "".join(str(s) for s in refine_np(x, np.array([0, len(mask)]), True, 0.3, max_gap, W, RADIUS)[1][:, 0])


def test_state_codes_on_a_hand_written_mask():
    g, g1 = "." * MAX_GAP, "." * (MAX_GAP + 1)
    assert states("uu" + g + "uu") == "00" + "1" * MAX_GAP + "00"                  # a gap of max_gap frames is filled
    assert states("uu" + g1 + "uu") == "00" + "3" * (MAX_GAP + 1) + "00"           # one frame more is left
    assert states(g + "uuu") == "2" * MAX_GAP + "000"                             # a leading run of max_gap is held
    assert states(g1 + "uuu") == "3" * (MAX_GAP + 1) + "000"
    assert states("uuu" + g) == "000" + "2" * MAX_GAP                             # a trailing run
    assert states("uuu" + g1) == "000" + "3" * (MAX_GAP + 1)
    assert states(g + "u" + g + "u" + g1) == "2" * MAX_GAP + "0" + "1" * MAX_GAP + "0" + "3" * (MAX_GAP + 1)
    assert states("....") == "3333" and states(".") == "3"                        # no usable frame: neither a leading nor a trailing run
    assert states("u") == "0" and states("u.") == "02" and states(".u") == "20" and states("uu") == "00"
    assert states("") == ""


def test_filled_values_on_a_hand_written_track():
    x = mask_track("..u...u.")
    x[2, 0, :2], x[6, 0, :2] = (100.0, 50.0), (108.0, 30.0)
    out, st = refine_np(x, np.array([0, 8]), True, 0.3, MAX_GAP, W, 0)
    assert st[:, 0].tolist() == [HELD, HELD, USABLE, INTERPOLATED, INTERPOLATED, INTERPOLATED, USABLE, HELD]
    assert out[:, 0, 0].tolist() == [100.0, 100.0, 100.0, 102.0, 104.0, 106.0, 108.0, 108.0]
    assert out[:, 0, 1].tolist() == [50.0, 50.0, 50.0, 45.0, 40.0, 35.0, 30.0, 30.0]
    assert same_bits(out[..., 2], x[..., 2])                                       # a filled joint keeps its low score


def test_tracks_of_no_one_and_two_frames():
    x = keypoints(3, seed=4)
    out, st = refine_np(x, np.array([0, 0, 1, 3]), True, 0.3, MAX_GAP, W, RADIUS)
    assert same_bits(out, x) and (st == USABLE).all()                              # r = 0 in every frame


def test_a_constant_track_with_gaps_comes_back_bit_for_bit():
    x = keypoints(80, value=np.float32(123.456))
    x[10:14, 0, 2] = 0.1                                                           # interpolated between equal values
    x[:3, 1, 2] = x[-2:, 1, 2] = 0.1                                               # held
    x[30:50, 2, 2] = 0.1                                                           # left: its positions are the constant as well
    out, st = refine_np(x, np.array([0, 80]), True, 0.3, MAX_GAP, W, RADIUS)
    assert same_bits(out, x)
    assert all((st == s).any() for s in (USABLE, INTERPOLATED, HELD, LEFT))


def test_first_and_last_frame_of_every_track_come_back_as_they_are():
    x = keypoints(60, seed=1)
    off = np.array([0, 1, 3, 20, 20, 60])
    out, _ = refine_np(x, off, True, 0.3, MAX_GAP, W, RADIUS)
    ends = sorted(set(off[:-1].tolist()) | set((off[1:] - 1).tolist()))
    assert same_bits(out[ends], x[ends])
    assert not same_bits(out[5:15], x[5:15])                                       # ... and the frames between them are smoothed


def test_an_integer_ramp_comes_back_exactly():
    n = 120
    x = keypoints(n, value=0.0)
    f = np.arange(n, dtype=np.float32)
    x[:, 0, 0], x[:, 0, 1] = 100.0 + f, 400.0 - 2.0 * f
    x[:, 1, 0], x[:, 1, 1] = 64.0 + 3.0 * f, 900.0 - f
    x[:, 2, 0], x[:, 2, 1] = 200.0 + 2.0 * f, 128.0 + f
    want = x.copy()
    for f0, g in ((20, 1), (40, 3), (70, 7)):                                      # gaps whose b - a is a power of two: t is exact
        x[f0:f0 + g, 1, :] = (7000.0, -7000.0, 0.05)
    out, st = refine_np(x, np.array([0, n]), True, 0.3, 8, W, RADIUS)
    assert (st[:, 1] == INTERPOLATED).sum() == 11 and (st[:, [0, 2]] == USABLE).all()
    assert same_bits(out[..., :2], want[..., :2])                                  # the ends and the narrow windows beside them included
    assert same_bits(out[..., 2], x[..., 2])


def test_max_gap_zero_fills_nothing():
    x, _, gated = synthetic_track(200, 5, seed=3)
    out, st = refine_np(x, np.array([0, 200]), True, 0.3, 0, W, RADIUS)
    assert gated.any() and not ((st == INTERPOLATED) | (st == HELD)).any()
    assert same_bits(out[gated], x[gated])                                         # an unknown joint is copied through


def test_radius_zero_is_the_gap_fill_alone():
    x, _, _ = synthetic_track(200, 5, seed=4)
    off = np.array([0, 90, 200])
    filled, st = refine_np(x, off, True, 0.3, 15, W, RADIUS, filled=True)
    out, st0 = refine_np(x, off, True, 0.3, 15, weights(None)[0], 0)
    assert same_bits(out, filled) and np.array_equal(st, st0) and (st == INTERPOLATED).any()


def test_a_track_alone_equals_the_track_in_a_batch_and_inputs_are_not_written():
    x, _, _ = synthetic_track(300, 4, seed=5)
    x[150:153] = np.nan
    off = np.array([0, 40, 41, 41, 170, 300])
    keep, keep_off = x.copy(), off.copy()
    out, st = refine_np(x, off, True, 0.3, 15, W, RADIUS)
    for lo, hi in zip(off[:-1], off[1:]):
        o1, s1 = refine_np(x[lo:hi], np.array([0, hi - lo]), True, 0.3, 15, W, RADIUS)
        assert same_bits(o1, out[lo:hi]) and np.array_equal(s1, st[lo:hi])
    assert same_bits(x, keep) and np.array_equal(off, keep_off)


def test_poses_are_gated_by_non_finite_values_alone():
    x = keypoints(30, seed=6)                                                      # three channels, none of them a score
    x[10:12, 0, 1], x[20, 1, 2] = np.nan, np.inf
    out, st = refine_np(x, np.array([0, 30]), False, 0.3, 15, W, RADIUS)
    assert (st[10:12, 0] == INTERPOLATED).all() and st[20, 1] == INTERPOLATED and (st != USABLE).sum() == 3
    assert np.isfinite(out).all()


# ---- the synthetic track (tests/refine_ref.synthetic_track): 600 frames, 17 joints, coordinates up to about 900 px ----
@pytest.fixture(scope="module")
def synthetic():
    x, truth, gated = synthetic_track()
    off = np.array([0, x.shape[0]])
    o32, st = refine_np(x, off, True, 0.3, 15, W, RADIUS)
    return x, truth, gated, off, o32, st


def test_fp32_against_the_same_statements_in_fp64(synthetic):
    """Measured 4.1e-5 px (coordinates up to 898 px, whose fp32 spacing is 6.1e-5); the bar is four times that, the convention of tests/test_smooth_cpu.py."""
    x, _, _, off, o32, st = synthetic
    o64, st64 = refine_np(x, off, True, 0.3, 15, W, RADIUS, ft=np.float64)
    err = np.abs(o32[..., :2].astype(np.float64) - o64[..., :2]).max()
    print(f"fp32 against fp64: {err:.3e} px")
    assert np.array_equal(st, st64)
    assert err <= 4 * 4.1e-5


def test_the_rule_beats_the_causal_filter_in_gaps_and_the_raw_input_elsewhere(synthetic):
    """A sanity check of the rule, not a quality claim: there is no footage here.  Measured: gated joint-frames 3.99 px against smooth_tracks' 25.7 px; usable
    joint-frames 1.25 px against the raw input's 1.99 px."""
    x, truth, gated, off, o32, st = synthetic

    def rms(a, m):
        return float(np.sqrt(((a[..., :2].astype(np.float64) - truth)[m] ** 2).mean()))

    causal = smooth_ref.tracks_np(smooth_ref.params(), x, off, True)
    print(f"gated: {rms(o32, gated):.2f} px, smooth_tracks {rms(causal, gated):.2f} px; usable: {rms(o32, ~gated):.2f} px, raw {rms(x, ~gated):.2f} px")
    assert 0.05 < gated.mean() < 0.2 and (st[gated] == INTERPOLATED).all()
    assert rms(o32, gated) < rms(causal, gated)
    assert rms(o32, ~gated) < rms(x, ~gated)
