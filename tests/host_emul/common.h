// Host stand-in for csrc/common.h, for the k_loss.hip build only (a copy of the kernel in the build directory finds this file, not the real header beside the
// original): the two names csrc/k_loss.hip and k_loss3 take from it.  reduce64 adds in the device function's order: its four DPP steps (quad xor 1, quad xor 2,
// mirror within 8, mirror within 16) pair every lane with one whose partial sum over the lanes already covered is the same set's, so each is the xor butterfly
// of that width, and fp32 addition commutes.
#pragma once
#include <hip/hip_runtime.h>
#define KASF_J 17
inline float reduce64(float v) {
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
