"""Constant limb lengths without a GPU: the fp32 restatement of include/kasf.h's rule (tests/bones_ref.py) against fp64, what the stage does to a synthetic
track, and the Python-side refusals of kasportsformer_amd.bones, which are raised before the library is loaded or anything is launched.

The bound on a scaled bone.  With eps = 2^-24 (half an ulp, relative) and v = x[child] - x[parent] as the walk rounded it:
  l' = sqrtf((vx vx + vy vy) + vz vz) = |v| (1 + d_l): the three squares err by eps each and weigh vx^2 / |v|^2 ... which sum to 1, the two additions by eps each,
       the root halves that and rounds once more;
  s  = L / l' (1 + d_1), |d_1| <= eps;   w_i = v_i s (1 + d_2i), |d_2i| <= eps, so |w| = L (1 + d_1 + d_2 - d_l) to first order;
  y[child]_i = (y[parent]_i + w_i)(1 + d_3i), |d_3i| <= eps: the difference y[child] - y[parent], formed exactly in fp64, is w plus a vector of norm at most
       sqrt(3) eps |y[child]|inf.
The issue's bound is 4 eps L + 2 sqrt(3) eps max(|y_p|inf, |y_c|inf): two roundings for s and the product, two more for l', one on the sum with a factor 2 to
spare.  (The first-order worst case of d_l is 2.5 eps, so all roundings at their extreme and aligned would give 4.5 eps L; a rounding error of eps needs a
significand next to a power of two, and the cases here stay below 4 eps L with room.  The bound is held as set, on every scaled bone of every case.)
Directions: w_i / |w| differs from v_i / |v| by d_2i only, and the sum adds sqrt(3) eps |y_c|inf / L: the same order."""
import numpy as np
import pytest
import torch

from tests import bones_ref as R


def test_fp32_walk_holds_the_fp64_length_bound_and_keeps_directions():
    worst_len, worst_dir = -np.inf, 0.0
    for seed, (scale, shift) in enumerate([(1.0, 0.0), (1.0, 30.0), (1000.0, 0.0), (1e-3, 1.0)]):
        x = (R.synthetic_track(200, 0.05, seed) * np.float32(scale) + np.float32(shift)).astype(np.float32)
        off = np.array([0, 200])
        for symmetric in (False, True):
            L, n = R.median_np(x, off)
            assert (n == 200).all()
            table = R.symmetric_np(L) if symmetric else L
            y = R.apply_np(x, off, L, symmetric)
            worst_len = max(worst_len, R.length_excess(y, table[0].astype(np.float64), np.ones((200, 16), bool)))
            # directions: the unit vectors of the bones before and after, in fp64
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            vx, vy = x64[:, R.CHILDREN] - x64[:, R.PARENTS], y64[:, R.CHILDREN] - y64[:, R.PARENTS]
            ux, uy = vx / np.linalg.norm(vx, axis=-1, keepdims=True), vy / np.linalg.norm(vy, axis=-1, keepdims=True)
            reach = np.maximum(np.abs(y64[:, R.CHILDREN]).max(-1), np.abs(y64[:, R.PARENTS]).max(-1))
            bound = 4 * R.EPS + 2 * np.sqrt(3) * R.EPS * reach / table[0]
            worst_dir = max(worst_dir, float((np.linalg.norm(ux - uy, axis=-1) / bound).max()))
            assert np.array_equal(y[:, 0].view(np.uint32), x[:, 0].view(np.uint32))              # the root stays where it was
    print(f"largest (length error - bound): {worst_len:.3e}; largest direction change / bound: {worst_dir:.3f}")
    assert worst_len <= 0 and worst_dir <= 1


def test_fp32_medians_are_the_fp64_medians_rounded():
    x = R.synthetic_track(301, 0.05, 9)
    L, n = R.median_np(x, np.array([0, 100, 301]))
    x64 = x.astype(np.float64)
    l64 = np.linalg.norm(x64[:, R.CHILDREN] - x64[:, R.PARENTS], axis=-1)
    for p, (a, b) in enumerate(((0, 100), (100, 301))):
        want = np.sort(l64[a:b], axis=0)[(b - a - 1) // 2]
        assert np.abs(L[p] - want).max() <= 4 * R.EPS * want.max()           # 2.5 eps on the length; neighbours in the order may swap within that
    assert (n == [[100] * 16, [201] * 16]).all()


def test_the_two_texts_of_the_walk_give_the_same_bits():
    x, off = R.median_tracks()
    L, _ = R.median_np(x, off)
    L[:, 4] = 0
    for symmetric in (False, True):
        for tab in (L, L[7]):
            assert np.array_equal(R.apply_np(x, off, tab, symmetric).view(np.uint32), R.apply_arrays_np(x, off, tab, symmetric).view(np.uint32))


def test_symmetric_is_idempotent_and_takes_the_partner_of_a_zero():
    L = np.abs(np.random.default_rng(1).normal(size=(50, 16))).astype(np.float32)
    L[::3, 0], L[1::4, 13], L[2::5, 2], L[2::5, 5] = 0, 0, 0, 0
    S = R.symmetric_np(L)
    assert np.array_equal(R.symmetric_np(S).view(np.uint32), S.view(np.uint32))
    for a, b in R.PARTNERS:
        assert np.array_equal(S[:, a], S[:, b])
    assert np.array_equal(S[::3, 0], L[::3, 3]) and np.array_equal(S[2::5, 2], np.zeros_like(S[2::5, 2])) and np.array_equal(S[:, 6:10], L[:, 6:10])


def test_a_synthetic_track_gets_its_true_lengths_and_loses_its_limb_variance():
    """A fixed skeleton under random rotations with Gaussian joint noise of 1 cm: the medians recover the true lengths to within the noise, and the limb-length
    variance (loss_limb_var_calc's definition) falls to rounding level.  The figures are printed; the README quotes them as what they are, synthetic."""
    noise, n = 0.01, 600
    x = R.synthetic_track(n, noise, 4)
    off = np.array([0, n])
    L, _ = R.median_np(x, off)
    true = R.true_lengths()
    # a bone's length carries the noise of two joints along its direction: sigma sqrt(2); the median of n of them: sigma sqrt(2) sqrt(pi / 2) / sqrt(n); 5 sigma,
    # plus the bias of a length under transverse noise, 2 sigma^2 / l
    bound = 5 * noise * np.sqrt(2) * np.sqrt(np.pi / 2) / np.sqrt(n) + 2 * noise ** 2 / true
    assert (np.abs(L[0] - true) <= bound).all(), (np.abs(L[0] - true) / bound).max()
    y = R.apply_np(x, off, L, False)
    before, after = R.limb_var(x), R.limb_var(y)
    print(f"limb-length variance before {before:.3e} m^2, after {after:.3e} m^2; largest median error {np.abs(L[0] - true).max():.2e} m")
    assert before > 1e-4 and after < 1e-13                                   # (4 eps L)^2 with L < 0.5 m and |y| of a few metres: about 1e-14
    # breathing by a few percent before, nothing after
    l_before = np.linalg.norm(x[:, R.CHILDREN].astype(np.float64) - x[:, R.PARENTS], axis=-1)
    assert (l_before.std(0) / l_before.mean(0)).max() > 0.03


# ---- the Python side refuses before the library is loaded ----
@pytest.fixture()
def no_library(monkeypatch):
    from kasportsformer_amd import _lib

    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.setattr(_lib, "_lib", None)


def test_fix_and_lengths_refuse_before_the_library_is_loaded(no_library):
    import kasportsformer_amd as K
    ok = np.zeros((6, 17, 3), np.float32)
    for fn in (K.fix_bone_lengths, K.bone_lengths):
        with pytest.raises(ValueError, match=r"\[N,17,3\]"):
            fn(np.zeros((6, 16, 3), np.float32))                 # J != 17
        with pytest.raises(ValueError, match=r"\[N,17,3\]"):
            fn(np.zeros((6, 17, 2), np.float32))
        with pytest.raises(ValueError, match=r"\[N,17,3\]"):
            fn(np.zeros((17, 3), np.float32))
        with pytest.raises(ValueError, match=r"\[P,N,17,3\]"):
            fn(np.zeros((1, 1, 6, 17, 3), np.float32))
        with pytest.raises(ValueError, match="packed tracks"):
            fn(np.zeros((2, 3, 17, 3), np.float32), offsets=[0, 2])
        with pytest.raises(ValueError, match="tracks of"):
            fn([np.zeros((2, 3, 17, 3), np.float32)])
        with pytest.raises(TypeError):
            fn(ok.astype(np.float64))
        for bad in ([0, 7], [1, 6], [0, 4, 3, 6], [0.0, 6.0], [[0, 6]], []):
            with pytest.raises(ValueError, match="offsets must be integers"):
                fn(ok, offsets=bad)
        with pytest.raises(RuntimeError):
            fn(ok, device="cpu")
    with pytest.raises(ValueError, match=r"lengths must be \[16\] or \[2,16\]"):
        K.fix_bone_lengths(ok, offsets=[0, 2, 6], lengths=np.zeros((3, 16), np.float32))
    with pytest.raises(ValueError, match="lengths must be"):
        K.fix_bone_lengths(ok, lengths=np.zeros(17, np.float32))
    with pytest.raises(TypeError):
        K.fix_bone_lengths(ok, lengths=np.zeros(16, np.float64))
    with pytest.raises(TypeError, match="symmetric must be a bool"):
        K.fix_bone_lengths(ok, symmetric=1)
    with pytest.raises(TypeError, match="return_lengths must be a bool"):
        K.fix_bone_lengths(ok, return_lengths="yes")
    assert K.fix_bone_lengths([]) == []


def test_a_tensor_on_another_device_is_refused(no_library, monkeypatch):
    """No machine of the CPU tests has two GPUs: a stand-in with a tensor's shape that says it lives on cuda:1 goes through the real checks."""
    from kasportsformer_amd import bones

    class Elsewhere:
        shape, is_cuda, device = (6, 17, 3), True, torch.device("cuda:1")

        def dim(self):
            return 3
    monkeypatch.setattr(bones, "_pose_rows", lambda a, who: a)
    for fn in (bones.fix_bone_lengths, bones.bone_lengths):
        with pytest.raises(RuntimeError, match="asked for cuda:0"):
            fn(Elsewhere(), device="cuda:0")
    f = object.__new__(bones.BoneLengthFilter)
    f.__dict__.update(tracked=False, slots=4, streams=None, track_slots=None, R=None, device=torch.device("cuda:0"))
    with pytest.raises(RuntimeError):
        f.push(torch.zeros((4, 17, 3), device="meta"))


def test_filter_refuses_before_the_library_is_loaded(no_library):
    import kasportsformer_amd as K
    F = K.BoneLengthFilter
    with pytest.raises(ValueError, match="not both"):
        F(slots=4, streams=2)
    with pytest.raises(ValueError, match="give slots="):
        F()
    for bad in (0, -1, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="window"):
            F(slots=4, window=bad)
    for bad in (1.5, True, "8"):
        with pytest.raises(TypeError, match="window"):
            F(slots=4, window=bad)
    with pytest.raises(TypeError, match="symmetric must be a bool"):
        F(slots=4, symmetric=0)
    with pytest.raises(ValueError, match="slots"):
        F(slots=0)
    with pytest.raises(ValueError, match="rows must be one of"):
        F(streams=1, track_slots=4, rows="people")
    with pytest.raises(ValueError, match="track_slots"):
        F(streams=1, track_slots=65)
    with pytest.raises(RuntimeError):
        F(slots=4, device="cpu")


def test_push_and_reset_refuse_before_any_launch(no_library):
    """The checks push and reset make, on an object laid out as the constructor leaves it (the constructor itself needs a GPU)."""
    import kasportsformer_amd as K
    from kasportsformer_amd import bones

    def bare(**kw):
        f = object.__new__(K.BoneLengthFilter)
        f.__dict__.update(dict(tracked=False, slots=4, streams=None, track_slots=None, R=None, device=torch.device("cuda:0"), window=8, symmetric=False), **kw)
        return f
    f = bare()
    for shape in ((3, 17, 3), (4, 16, 3), (4, 17, 2), (4, 17, 3, 1)):
        with pytest.raises(ValueError, match="expected rows"):
            f.push(np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="distinct"):
        f.push(np.zeros((2, 17, 3), np.float32), slots=[1, 1])
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        f.push(np.zeros((1, 17, 3), np.float32), slots=[4])
    with pytest.raises(TypeError, match="takes slots=, not a TrackResult"):
        f.push(np.zeros((4, 17, 3), np.float32), object())
    with pytest.raises(TypeError):
        f.push(np.zeros((4, 17, 3), np.float64))
    with pytest.raises(TypeError, match="reset by slots"):
        f.reset(streams=[0])
    with pytest.raises(ValueError):
        f.reset(slots=[9])
    t = bare(tracked=True, slots=8, streams=2, track_slots=4, R=2)
    with pytest.raises(TypeError, match="TrackResult, not slots="):
        t.push(np.zeros((4, 17, 3), np.float32), slots=[0])
    with pytest.raises(TypeError, match="track .* is required"):
        t.push(np.zeros((2, 2, 17, 3), np.float32))
    with pytest.raises(ValueError, match="expected rows"):
        t.push(np.zeros((2, 3, 17, 3), np.float32), object())
    with pytest.raises(TypeError, match="reset by streams="):
        t.reset(slots=[0])
    with pytest.raises(ValueError):
        t.reset(streams=[2])
    assert bones.BONE_PARENTS == R.PARENTS and bones.BONE_PARTNERS == R.PARTNERS


def test_the_bone_table_is_the_models_own():
    from kasportsformer_amd import draw
    segs = {tuple(sorted(s[:2])) for s in draw.H36M_SEGMENTS}
    assert segs == {(p, k + 1) for k, p in enumerate(R.PARENTS)}
