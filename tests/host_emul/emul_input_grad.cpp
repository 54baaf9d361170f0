// csrc/k_input_grad.hip compiled for the host (tests/test_input_grad_host_cpu.py): a copy of the kernel in the build directory, so that its #include "common.h"
// finds the stand-in of this directory.  The kernel takes KASF_J and gelu_and_grad from common.h; the stand-in has the first, and the second -- the device's is
// built on v_exp_f32 / v_rcp_f32 -- is libm's here: GELU(x) = x Phi(x), GELU'(x) = Phi(x) + x pdf(x).  So the host build shows the kernel's logic, its tables, its
// staging and its summation order, not the device's GELU' arithmetic (tests/test_gpu_input_grad.py).
// With -DEMUL_INPUT_GRAD_MAIN the file is a stand-alone program for a sanitizer build (the command is in the test file's docstring).
#include "common.h"
template <typename T = float> inline void gelu_and_grad(float x, float& y, float& dy) {
    const float Phi = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    y = x * Phi;
    dy = Phi + x * 0.3989422804014327f * expf(-0.5f * x * x);
}
#include "kernels.h"
#include "k_input_grad.hip"
// off: a KasfProOff as int64 words (mlp [51][4] | embed_w [3] | embed_b [3] | pos [3]); returns the launches made
extern "C" int emul_input_grad(const float* x, const float* params, const int64_t* off, const float* dx_joint3, const float* dbone3, const float* dlimb3, float* dx,
                               int64_t frames) {
    static_assert(sizeof(KasfProOff) == (51 * 4 + 9) * sizeof(int64_t), "KasfProOff is 213 int64 words");
    g_launches = 0;
    kasf_launch_input_grad(nullptr, x, params, reinterpret_cast<const KasfProOff*>(off), dx_joint3, dbone3, dlimb3, dx, frames);
    return g_launches;
}

#ifdef EMUL_INPUT_GRAD_MAIN
#include <cstdio>
// frames 1, 3 (every subset of the three gradients) and 2,049 (one past the grid's first walk; all three), exact-size heap buffers so that a read or write one float past
// any of them is an AddressSanitizer report; planted: a zero-length bone and an all-zero frame.  Prints the sum of every dx as a checksum.
int main() {
    KasfProOff off{};
    std::vector<float> params;
    const int n_of[17] = {3, 3, 2, 2, 3, 3, 4, 4, 4, 4, 3, 4, 4, 4, 4, 2, 2};
    unsigned seed = 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 8388608.0f - 1.0f; };
    for (int t = 0; t < 51; ++t) {
        const int sizes[4] = {16 * n_of[t / 3], 16, 16, 1};
        for (int k = 0; k < 4; ++k) {
            off.mlp[t][k] = (int64_t)params.size();
            for (int e = 0; e < sizes[k]; ++e) params.push_back(rnd());
        }
    }
    double checksum = 0.0;
    for (int64_t frames : {(int64_t)1, (int64_t)3, (int64_t)2049}) {
        const size_t n = (size_t)frames * 51;
        std::vector<float> x(n), g[3] = {std::vector<float>(n), std::vector<float>(n), std::vector<float>(n)}, dx(n);
        for (size_t e = 0; e < n; ++e) { x[e] = rnd(); for (auto& v : g) v[e] = rnd(); }
        x[2 * 3] = x[3 * 3]; x[2 * 3 + 1] = x[3 * 3 + 1];                     // bone 2 of frame 0: child 2 == parent 3
        if (frames > 2) for (int e = 0; e < 51; ++e) x[2 * 51 + e] = 0.f;       // frame 2: every bone has length zero
        for (int mask = frames > 3 ? 7 : 0; mask < 8; ++mask) {   // every operand set at the small sizes, all three gradients at the large one
            std::fill(dx.begin(), dx.end(), NAN);
            const int made = emul_input_grad(x.data(), params.data(), reinterpret_cast<const int64_t*>(&off), mask & 1 ? g[0].data() : nullptr,
                                             mask & 2 ? g[1].data() : nullptr, mask & 4 ? g[2].data() : nullptr, dx.data(), frames);
            if (made != 1) { std::printf("FAILED: %d launches\n", made); return 1; }
            for (float v : dx) {
                if (!std::isfinite(v)) { std::printf("FAILED: a non-finite or unwritten dx (frames %lld, mask %d)\n", (long long)frames, mask); return 1; }
                checksum += v;
            }
        }
    }
    std::printf("emul_input_grad: frames 1, 3, 2049 done, checksum %.9g\n", checksum);
    return 0;
}
#endif
