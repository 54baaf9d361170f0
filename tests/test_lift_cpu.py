"""Host side of lifting a 2-D track (kasportsformer_amd/lift.py): the window plan against the reference demo's tables
(tests/golden/lift_tables.npz, written by make_lift_golden.py from demo/demo.py:132-156) and a restatement of its clip cutting,
the device-free window count of the C-ABI, and the keypoint loader of the CLI."""
import os
import pickle

import numpy as np
import pytest

from kasportsformer_amd.lift import load_keypoints, window_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("T", [27, 81, 243])
def test_resample_tables_match_the_demo(T):
    fx = np.load(os.path.join(GOLDEN, "lift_tables.npz"))
    r_ref, fp_ref = fx[f"resample_T{T}"], fx[f"first_pos_T{T}"]
    for L in range(1, T):
        starts, lengths, r, fp = window_plan(L, T)
        assert starts.tolist() == [0] and lengths.tolist() == [L]
        assert r.dtype == np.int32 and np.array_equal(r, r_ref[L - 1]), L
        assert fp.dtype == np.int32 and np.array_equal(fp, fp_ref[L - 1, :L]), L
        # the tail window of a longer track uses the same tables
        _, lengths2, r2, fp2 = window_plan(3 * T + L, T)
        assert lengths2[-1] == L and np.array_equal(r2, r) and np.array_equal(fp2, fp)


def _expected_windows(n, T, s):
    if n == 0:
        return [], []
    if n <= T:
        return [0], [n]
    if s == T:                                       # turn_into_clips: range(0, n, T) and the slice lengths
        starts = list(range(0, n, T))
        return starts, [len(range(n)[a:a + T]) for a in starts]
    starts = []
    a = 0
    while a + T < n:
        starts.append(a)
        a += s
    starts.append(n - T)
    return starts, [T] * len(starts)


@pytest.mark.parametrize("T", [27, 81])
@pytest.mark.parametrize("n", [0, 1, 26, 27, 28, 53, 54, 55, 200])
def test_window_starts_lengths_and_the_library_count(n, T):
    from kasportsformer_amd import _lib
    lib = _lib.load()
    for s in sorted({T, T // 3, 1}):
        starts, lengths, r, fp = window_plan(n, T, s)
        want_s, want_l = _expected_windows(n, T, s)
        assert starts.tolist() == want_s and lengths.tolist() == want_l, (n, T, s)
        assert lib.kasf_lift_window_count(n, T, s) == len(starts), (n, T, s)
        short = bool(len(want_l)) and want_l[-1] < T
        assert (r is None) == (not short) and (fp is None) == (not short)
        if s < T and n > T:
            cover = np.zeros(n, int)
            for a in starts:
                cover[a:a + T] += 1
            assert cover.min() >= 1 and np.all(np.diff(starts) > 0)


def test_reference_mode_handles_exact_multiples():
    """turn_into_clips (demo.py:138-156) raises UnboundLocalError at N = k T with k > 1; the plan gives k full windows."""
    starts, lengths, r, fp = window_plan(54, 27)
    assert starts.tolist() == [0, 27] and lengths.tolist() == [27, 27] and r is None and fp is None


def test_invalid_plans_are_refused():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    for n, T, s in ((10, 27, 0), (10, 27, 28), (-1, 27, 27), (10, 0, 1)):
        with pytest.raises(ValueError):
            window_plan(n, T, s)
        assert lib.kasf_lift_window_count(n, T, s) < 0
        assert lib.kasf_last_error()
    # the device entries refuse the same arguments and a missing table before touching any pointer
    assert lib.kasf_lift_windows(None, 1, 10, 1280.0, 720.0, 27, 0, None, 1, None, None) == 2
    assert lib.kasf_lift_windows(None, 1, 10, 1280.0, 720.0, 27, 27, None, 1, None, None) == 2
    assert lib.kasf_lift_stitch(None, 1, 1, 20, 27, 27, None, None, None) == 2
    assert lib.kasf_lift_windows(None, 1, 0, 1280.0, 720.0, 27, 27, None, 1, None, None) == 0       # n = 0: nothing to do


class _Evil:
    def __reduce__(self):
        return (os.system, ("true",))


def test_keypoint_loader_reads_numpy_and_refuses_other_globals(tmp_path):
    kp = np.random.default_rng(0).uniform(0, 1000, (2, 5, 17, 3)).astype(np.float32)
    p = tmp_path / "keypoints2d.pkl"
    p.write_bytes(pickle.dumps(kp))
    assert np.array_equal(load_keypoints(str(p)), kp)
    q = tmp_path / "keypoints2d.npy"
    np.save(q, kp)
    assert np.array_equal(load_keypoints(str(q)), kp)
    bad = tmp_path / "bad.pkl"
    bad.write_bytes(pickle.dumps({"kp": kp, "x": _Evil()}))
    with pytest.raises(pickle.UnpicklingError):
        load_keypoints(str(bad))


class _NumpyCallable:
    """A pickle that REDUCEs a numpy function which executes a string: admitted by a "module starts with numpy" rule."""

    def __reduce__(self):
        from numpy.testing._private.utils import runstring
        return (runstring, ("import builtins; builtins.KASF_LIFT_PICKLE_RAN = True", {}))


def test_keypoint_loader_refuses_numpy_callables_before_they_run(tmp_path):
    import builtins
    bad = tmp_path / "numpy_callable.pkl"
    bad.write_bytes(pickle.dumps(_NumpyCallable()))
    with pytest.raises(pickle.UnpicklingError):
        load_keypoints(str(bad))
    assert not hasattr(builtins, "KASF_LIFT_PICKLE_RAN")


@pytest.mark.parametrize("protocol", [2, 3, 4, 5])
def test_keypoint_loader_reads_every_pickle_protocol(tmp_path, protocol):
    kp = np.random.default_rng(1).uniform(0, 1000, (1, 7, 17, 3)).astype(np.float32)
    p = tmp_path / "keypoints2d.pkl"
    p.write_bytes(pickle.dumps(kp, protocol=protocol))
    assert np.array_equal(load_keypoints(str(p)), kp)
    obj = tmp_path / "objects.pkl"                       # an object array needs globals beyond the array's own
    obj.write_bytes(pickle.dumps(np.array([_Evil()], dtype=object), protocol=protocol))
    with pytest.raises(pickle.UnpicklingError):
        load_keypoints(str(obj))
