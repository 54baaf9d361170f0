"""Host side of lifting many tracks of different lengths in one call (kasportsformer_amd.lift_tracks): the ragged window plan of the C-ABI
(kasf_lift_ragged_plan) and of the host code against window_plan track by track, their refusals, and the multi-track keypoint files of the CLI."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from kasportsformer_amd.lift import load_keypoints, ragged_plan, window_plan


def _c_plan(lengths, T, s):
    from kasportsformer_amd import _lib
    n = np.asarray(lengths, np.int64)
    wf = np.full(len(n) + 1, -7, np.int64)
    total = _lib.load().kasf_lift_ragged_plan(n.ctypes.data_as(C.c_void_p), len(n), T, s, wf.ctypes.data_as(C.c_void_p))
    return total, wf


@pytest.mark.parametrize("T", [27, 81])
@pytest.mark.parametrize("which", ["T", "third", "one"])
def test_ragged_plan_is_window_plan_per_track(T, which):
    s = {"T": T, "third": T // 3, "one": 1}[which]
    lengths = [0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 5, 1000]
    rng = np.random.default_rng(T + s)
    for order in (lengths, [int(n) for n in rng.permutation(lengths)], lengths[::-1] + lengths):
        win_first, resample, first_pos = ragged_plan(order, T, s)
        assert win_first.dtype == np.int64 and resample.dtype == np.int32 and first_pos.dtype == np.int32
        assert win_first.shape == (len(order) + 1,) and resample.shape == first_pos.shape == (len(order), T)
        want = [0]
        for p, n in enumerate(order):
            starts, _, r, fp = window_plan(n, T, s)
            want.append(want[-1] + len(starts))
            if r is not None:
                assert np.array_equal(resample[p], r) and np.array_equal(first_pos[p, :len(fp)], fp), (n, T, s)
        assert win_first.tolist() == want
        total, wf = _c_plan(order, T, s)
        assert total == want[-1] and wf.tolist() == want, (order, T, s)


def test_ragged_plan_of_no_tracks():
    win_first, resample, first_pos = ragged_plan([], 27)
    assert win_first.tolist() == [0] and resample.shape == first_pos.shape == (0, 27)
    total, wf = _c_plan([], 27, 27)
    assert total == 0 and wf.tolist() == [0]


def test_ragged_plan_refusals():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    for lengths, T, s in (([10], 27, 0), ([10], 27, 28), ([10], 0, 1), ([10, -1, 5], 27, 27), ([-3], 27, 9)):
        with pytest.raises(ValueError):
            ragged_plan(lengths, T, s)
        total, wf = _c_plan(lengths, T, s)
        assert total < 0 and lib.kasf_last_error()
        assert wf.tolist() == [-7] * len(wf), "nothing is written on a refusal"
    assert _c_plan([10], 257, 1)[0] < 0                      # the library's T range, [1, 256]
    assert lib.kasf_lift_ragged_plan(None, 1, 27, 27, None) < 0
    assert lib.kasf_lift_ragged_plan(None, -1, 27, 27, None) < 0


def test_device_entries_refuse_before_touching_a_pointer():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    win = lib.kasf_lift_windows_ragged
    assert win(None, None, None, 1, 10, 1, None, None, 27, 0, None, 1, None, None) == 2           # stride 0
    assert win(None, None, None, 1, 10, 1, None, None, 27, 27, None, 1, None, None) == 2          # null pointers
    assert win(None, None, None, 1, 0, 1, None, None, 27, 27, None, 1, None, None) == 2           # a window without frames
    assert win(None, None, None, 0, 5, 1, None, None, 27, 27, None, 1, None, None) == 2           # frames without a track
    assert win(None, None, None, 1, 5, 6, None, None, 27, 27, None, 1, None, None) == 2           # more windows than frames
    assert win(None, None, None, 2, 0, 0, None, None, 27, 27, None, 1, None, None) == 0           # nothing to do
    st = lib.kasf_lift_stitch_ragged
    assert st(None, 1, None, None, 1, 20, 1, 27, 27, None, None, None) == 2
    assert st(None, 1, None, None, 1, 20, 21, 27, 27, None, None, None) == 2
    assert st(None, 1, None, None, -1, 0, 0, 27, 27, None, None, None) == 2
    assert st(None, 1, None, None, 3, 0, 0, 27, 27, None, None, None) == 0


def test_lift_tracks_needs_a_gpu_model():
    import kasportsformer_amd as K
    m = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=27, compute_dtype="fp32")
    with pytest.raises(RuntimeError, match="lift_tracks"):
        K.lift_tracks(m, [np.zeros((5, 17, 3), np.float32)], 1280, 720)


class _Evil:
    def __reduce__(self):
        return (os.system, ("true",))


def test_keypoint_loader_reads_track_lists_and_npz(tmp_path):
    g = np.random.default_rng(0)
    tracks = [g.uniform(0, 1000, (n, 17, 3)).astype(np.float32) for n in (5, 0, 61, 1)]
    for protocol in (3, 5):                              # (protocol 2 writes an empty array's bytes through a global the loader refuses)
        for seq in (list, tuple):
            p = tmp_path / f"tracks_{protocol}_{seq.__name__}.pkl"
            p.write_bytes(pickle.dumps(seq(tracks), protocol=protocol))
            got = load_keypoints(str(p))
            assert isinstance(got, list) and len(got) == len(tracks)
            assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(got, tracks))
    z = tmp_path / "tracks.npz"
    np.savez(z, b=tracks[0], a=tracks[1], c=tracks[2], d=tracks[3])     # file order, not name order
    got = load_keypoints(str(z))
    assert isinstance(got, list) and [a.shape[0] for a in got] == [5, 0, 61, 1]
    assert all(np.array_equal(a, b) for a, b in zip(got, tracks))
    one = tmp_path / "one.pkl"                                          # a single array keeps the single-array result
    one.write_bytes(pickle.dumps(tracks[2]))
    kp = load_keypoints(str(one))
    assert isinstance(kp, np.ndarray) and np.array_equal(kp, tracks[2])


def test_keypoint_loader_still_refuses_other_globals(tmp_path):
    kp = np.zeros((3, 17, 3), np.float32)
    bad = tmp_path / "bad.pkl"
    for obj in ([kp, _Evil()], (kp, {"x": _Evil()}), [np.array([_Evil()], dtype=object)]):
        bad.write_bytes(pickle.dumps(obj))
        with pytest.raises(pickle.UnpicklingError):
            load_keypoints(str(bad))
    bad.write_bytes(pickle.dumps([kp, 3]))                              # a list of something other than numeric arrays
    with pytest.raises(TypeError):
        load_keypoints(str(bad))
    obj = tmp_path / "objects.npz"
    np.savez(obj, a=kp, b=np.array([1, "x"], dtype=object))
    with pytest.raises(ValueError):                                     # object arrays in an .npz need pickles, which the loader does not allow
        load_keypoints(str(obj))
