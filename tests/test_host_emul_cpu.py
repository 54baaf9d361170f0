"""tests/host_emul/hip/hip_runtime.h on its own: every assertion of the host-compiled kernel tests (tests/test_*_host_cpu.py) rests on that stand-in modelling
the grid, the wave collectives, the dynamic LDS and the 16-bit types correctly.  Toy kernels with known answers (tests/host_emul/selftest.cpp), and the two
conversion classes against torch's conversion of the same fp32 bit patterns."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests.host_emul import build, vp


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build(tmp_path_factory, "host_emul_selftest", "selftest.cpp")


def test_every_index_of_a_3_x_2_grid_of_128_threads_appears_exactly_once(lib):
    rec = np.full((3 * 2 * 128, 9), -1, np.int32)
    lib.selftest_indices(vp(rec))
    assert (rec[:, 3:] == (3, 2, 1, 128, 1, 1)).all(), "gridDim and blockDim in every thread"
    assert sorted(map(tuple, rec[:, :3])) == sorted(itertools.product(range(3), range(2), range(128))), "(blockIdx.x, blockIdx.y, threadIdx.x)"


def ballot(lib, threads):
    out = np.full(threads, 0xDEAD, np.uint64)
    lib.selftest_ballot(threads, vp(out))
    return out


WAVE0 = sum(1 << l for l in range(64) if l % 3 == 0)
WAVE1 = sum(1 << l for l in range(64) if l % 2)


def test_ballot_gives_each_wave_of_a_128_thread_block_its_own_mask(lib):
    out = ballot(lib, 128)
    assert (out[:64] == WAVE0).all() and (out[64:] == WAVE1).all()


def test_ballot_of_a_half_wave_has_no_upper_bits(lib):
    ballot(lib, 128)                                   # leaves votes of threads 96..127 behind: lanes a block of 96 does not have
    out = ballot(lib, 96)
    assert (out[:64] == WAVE0).all() and (out[64:] == WAVE1 & 0xFFFFFFFF).all()


def test_shfl_xor_butterfly_sums_each_wave_alone(lib):
    out = np.full(128, np.nan, np.float32)
    lib.selftest_butterfly(vp(out))
    assert (out[:64] == sum(range(64))).all() and (out[64:] == sum(range(64, 128))).all()


def test_shfl_of_a_double_reaches_its_own_wave_only(lib):
    out = np.full(128, np.nan, np.float64)
    lib.selftest_broadcast(vp(out))
    assert (out[:64] == 5.5).all() and (out[64:] == 1005.5).all()


def test_syncthreads_or_three_in_a_row(lib):
    out = np.full((128, 3), -1, np.int32)
    lib.selftest_or(vp(out))
    assert (out == (1, 0, 1)).all(), "predicates: one thread, none, all"


@pytest.mark.parametrize("ask,write,want", [(100, 100, (1, 1, 0, 1)), (100, 101, (1, 1, 1, 1)), (0, 0, (1, 0, 0, 1))])
def test_dynamic_lds_is_exactly_what_the_launch_asked_for(lib, ask, write, want):
    """The one byte further lands in the host buffer's own canary area."""
    out = np.full(4, -1, np.int32)
    lib.selftest_lds(ask, write, vp(out))
    assert tuple(out) == want, "(launches, LDS asked for, overrun, HIP_DYNAMIC_SHARED and KASF_DYNAMIC_LDS name one buffer)"


def conversion_inputs():
    bits = np.random.default_rng(7).integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)
    special = [0.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1.5 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14,       # fp16 subnormals, their ties
               2.0 ** -149, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126,                                            # fp32 / bf16 subnormals
               1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23,  # exact ties and one ulp past
               65504.0, 65519.996, 65520.0, 3.3895313892515355e38, 3.3961775292304601e38, 3.4028234663852886e38, np.inf]                    # the largest finite values
    x = np.array(special, np.float32)
    return np.concatenate((bits.view(np.float32), x, -x, np.array([np.nan], np.float32)))


def test_the_16_bit_classes_convert_as_torch_does(lib):
    x = conversion_inputs()
    half, bf16 = np.zeros(x.size, np.uint16), np.zeros(x.size, np.uint16)
    lib.selftest_convert(vp(x), C.c_int64(x.size), vp(half), vp(bf16))
    t, nan = torch.from_numpy(x), np.isnan(x)
    assert nan.any() and (~nan).sum() > 99_000
    for got, dtype, inf_bits in ((half, torch.float16, 0x7C00), (bf16, torch.bfloat16, 0x7F80)):
        want = t.to(dtype).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got[~nan], want[~nan]), dtype
        assert ((got[nan] & 0x7FFF) > inf_bits).all(), "NaN goes to NaN"
