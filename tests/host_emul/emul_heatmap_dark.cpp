// csrc/k_heatmap.hip compiled for the host (tests/test_heatmap_dark_host_cpu.py): the DARK / UDP decode kernels behind the lockstep emulation.
#include <hip/hip_runtime.h>

// what k_heatmap.hip takes from HIP beyond the stand-in: the shuffles' width argument (always 64 there), the bit cast, and a half that can be read -- the
// stand-in's emu_half only rounds a float into one, the heatmap kernels only widen one, which is exact
template <class T> inline T __shfl_xor(T v, int off, int width) { (void)width; return __shfl_xor(v, off); }
inline float __uint_as_float(unsigned u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
struct read_half {
    uint16_t bits;
    explicit operator float() const {
        const uint32_t sign = (uint32_t)(bits & 0x8000u) << 16, e = (bits >> 10) & 31u, m = bits & 0x3ffu;
        if (e == 0) {                                          // zero or subnormal: m * 2^-24, exact in fp32
            const float v = (float)m * 5.9604644775390625e-08f;
            return sign ? -v : v;
        }
        return __uint_as_float(sign | (e == 31 ? 0x7f800000u | (m << 13) : ((e + 112u) << 23) | (m << 13)));
    }
};
#undef _Float16
#define _Float16 read_half

#include "kernels.h"
#include "k_heatmap.hip"

extern "C" void emul_heatmap_decode(const void* hm, const void* hmf, int dtype, int64_t n, int H, int W, const int* partner, int shift, const float* geom,
                                    int geom_kind, double aspect, int mode, const float* weights, int K, int udp, float* out, float* merged_out) {
    kasf_launch_heatmap_decode(nullptr, hm, hmf, dtype, n, H, W, partner, shift, geom, geom_kind, aspect, mode, weights, K, udp, out, merged_out);
}
extern "C" int emul_launches() { return g_launches; }
