// csrc/k_refine.hip compiled for the host (tests/test_refine_host_cpu.py).  w: the 33 weights.  Returns whether a block wrote past the LDS its launch asked for.
#include "kernels.h"
#include "k_refine.hip"
extern "C" int emul_refine(const float* x, const int64_t* offsets, int64_t N, int P, int J, int C, int has_score, float min_score, int max_gap, int radius,
                           const float* w, float* out, unsigned char* state) {
    KasfRefine p{min_score, max_gap, radius, {}};
    for (int k = 0; k <= kRefineMaxRadius; ++k) p.w[k] = w[k];
    g_lds_overrun = 0;
    kasf_launch_tracks_refine(nullptr, x, offsets, N, P, J, C, has_score, p, out, state);
    return g_lds_overrun;
}
