"""Host side of the online lift (kasportsformer_amd.StreamLifter): the window tables of the C-ABI (kasf_stream_tables) against the host's
stream_tables against window_plan row by row, the resample rule against numpy's linspace for every plan, and the refusals of the entry points."""
import ctypes as C

import numpy as np
import pytest

from kasportsformer_amd.lift import demo_resample, window_plan


def _c_tables(T, fill=-7):
    from kasportsformer_amd import _lib
    r = np.full((max(T, 0) + 1, max(T, 1)), fill, np.int32)
    fp = np.full_like(r, fill)
    rc = _lib.load().kasf_stream_tables(T, r.ctypes.data_as(C.c_void_p), fp.ctypes.data_as(C.c_void_p))
    return rc, r, fp


@pytest.mark.parametrize("T", [4, 27, 81, 256])
def test_tables_are_window_plan_row_by_row(T):
    from kasportsformer_amd.stream import stream_tables
    rc, c_r, c_fp = _c_tables(T)
    assert rc == 0
    r, fp = stream_tables(T)
    assert r.dtype == fp.dtype == np.int32 and r.shape == fp.shape == (T + 1, T)
    assert np.array_equal(c_r, r) and np.array_equal(c_fp, fp)
    assert not r[0].any() and not fp[0].any()
    assert np.array_equal(r[T], np.arange(T)) and np.array_equal(fp[T], np.arange(T))
    for n in range(1, T):
        starts, lengths, want_r, want_fp = window_plan(n, T)
        assert starts.tolist() == [0] and lengths.tolist() == [n] and len(want_fp) == n
        assert np.array_equal(c_r[n], want_r), n
        assert np.array_equal(c_fp[n, :n], want_fp) and not c_fp[n, n:].any(), n
        assert np.array_equal(c_r[n][c_fp[n, :n]], np.arange(n)), "first_pos leads back to every frame of the window"


def test_resample_rule_is_linspace_for_every_plan():
    """clamp(floor((double)t * ((double)n / (double)T)), 0, n - 1) against np.linspace(0, n, T, endpoint=False) (demo.py:132-136) for every
    1 <= n <= T <= 256: no mismatch, and every row is onto 0 .. n-1, so first_pos is total."""
    for T in range(1, 257):
        rc, r, fp = _c_tables(T)
        assert rc == 0
        for n in range(1, T + 1):
            assert np.array_equal(r[n], demo_resample(n, T)), (n, T)
            assert np.array_equal(np.unique(r[n]), np.arange(n)), (n, T)
            assert np.array_equal(r[n][fp[n, :n]], np.arange(n)) and np.all(np.diff(fp[n, :n]) > 0), (n, T)


def test_table_refusals_write_nothing():
    from kasportsformer_amd import _lib
    from kasportsformer_amd.stream import stream_tables
    lib = _lib.load()
    for T in (0, -3, 257):
        rc, r, fp = _c_tables(T)
        assert rc == 2 and lib.kasf_last_error()
        assert (r == -7).all() and (fp == -7).all(), "nothing is written on a refusal"
    keep = np.full((28, 27), -7, np.int32)
    assert lib.kasf_stream_tables(27, None, keep.ctypes.data_as(C.c_void_p)) == 2
    assert lib.kasf_stream_tables(27, keep.ctypes.data_as(C.c_void_p), None) == 2
    assert (keep == -7).all()
    with pytest.raises(ValueError):
        stream_tables(0)


def test_device_entries_refuse_before_touching_a_pointer():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    push = lib.kasf_stream_push                             # (frames, slots, K, S, T, ring, count, stream)
    assert push(None, None, 4, 4, 27, None, None, None) == 2            # null pointers
    assert push(None, None, 4, 4, 0, None, None, None) == 2             # T outside [1, 256]
    assert push(None, None, 4, 4, 257, None, None, None) == 2
    assert push(None, None, 5, 4, 27, None, None, None) == 2            # more pushed slots than slots
    assert push(None, None, -1, 4, 27, None, None, None) == 2
    assert push(None, None, 1, -1, 27, None, None, None) == 2
    assert push(None, None, 2, 4, 27, None, None, None) == 2            # a subset of the slots needs their ids
    assert push(None, None, 0, 4, 27, None, None, None) == 0            # nothing to do
    win = lib.kasf_stream_windows                           # (ring, count, slots, K, S, T, width, height, resample_tab, flip, x, stream)
    assert win(None, None, None, 4, 4, 27, None, None, None, 1, None, None) == 2
    assert win(None, None, None, 4, 4, 300, None, None, None, 1, None, None) == 2
    assert win(None, None, None, 5, 4, 27, None, None, None, 1, None, None) == 2
    assert win(None, None, None, 3, 4, 27, None, None, None, 0, None, None) == 2
    assert win(None, None, None, 0, 4, 27, None, None, None, 1, None, None) == 0
    emit = lib.kasf_stream_emit                             # (pred, flip, count, slots, K, S, T, first_pos_tab, back, n_out, out, stream)
    assert emit(None, 1, None, None, 4, 4, 27, None, 0, 1, None, None) == 2
    assert emit(None, 1, None, None, 4, 4, 27, None, 27, 1, None, None) == 2    # back outside [0, T - 1]
    assert emit(None, 1, None, None, 4, 4, 27, None, -1, 1, None, None) == 2
    assert emit(None, 1, None, None, 4, 4, 27, None, 0, 28, None, None) == 2    # more rows than a window has frames
    assert emit(None, 1, None, None, 4, 4, 27, None, 0, -1, None, None) == 2
    assert emit(None, 1, None, None, 9, 4, 27, None, 0, 1, None, None) == 2
    assert emit(None, 1, None, None, 4, 4, 0, None, 0, 1, None, None) == 2
    assert emit(None, 1, None, None, 4, 4, 27, None, 0, 0, None, None) == 0     # no rows asked for
    assert emit(None, 1, None, None, 0, 4, 27, None, 0, 1, None, None) == 0
    assert lib.kasf_last_error()


def test_abi_version_is_at_least_11():
    from kasportsformer_amd import _lib
    assert _lib.ABI_VERSION == _lib.load().kasf_version() >= 11       # the stream entries are ABI 11's; tests/test_cabi_cpu.py pins the current number
    assert all(n in _lib.SIGNATURES for n in ("kasf_stream_tables", "kasf_stream_push", "kasf_stream_windows", "kasf_stream_emit"))


def test_stream_lifter_needs_a_gpu_model():
    import kasportsformer_amd as K
    m = K.KASportsFormer(n_layers=1, num_heads=8, n_frames=27, compute_dtype="fp32")
    with pytest.raises(RuntimeError, match="StreamLifter"):
        K.StreamLifter(m, 1280, 720, slots=4)
