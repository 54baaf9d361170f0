// csrc/k_optim.hip compiled for the host (tests/test_optim_host_cpu.py).  kasf.h and k_adamw.inc are written into the build directory by the test: the public
// header as it is, and the ew_grid / k_adamw / kasf_launch_adamw text of csrc/k_misc.hip cut out as it is, for the bit comparison with the one-range update
// (its f32x4 is k_optim.hip's typedef).  The classes arrive with bc1 / bc2 filled in (the C-ABI forms them; the launcher takes them as they are).
#include "kernels.h"
#include "k_optim.hip"
#include "k_adamw.inc"
extern "C" int emul_adamw_segments(float* p, const float* g, float* m, float* v, const KasfOptChunk* chunks, int64_t n_chunks, const KasfAdamwClass* classes,
                                   int n_classes, float grad_scale, const float* clip, int grid_cap) {
    KasfAdamwClasses by_value{};
    for (int k = 0; k < n_classes; ++k) by_value.c[k] = classes[k];
    g_launches = 0;
    kasf_launch_adamw_segments(nullptr, p, g, m, v, chunks, n_chunks, by_value, grad_scale, clip, grid_cap);
    return g_launches;
}
extern "C" int emul_grad_norm(const float* g, const KasfOptChunk* chunks, int64_t n_chunks, double* partial, float grad_scale, float max_norm, float* out2,
                              int grid_cap) {
    g_launches = 0;
    kasf_launch_grad_norm(nullptr, g, chunks, n_chunks, partial, grad_scale, max_norm, out2, grid_cap);
    return g_launches;
}
extern "C" int emul_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2,
                          float grad_scale) {
    g_launches = 0;
    kasf_launch_adamw(nullptr, p, g, m, v, n, lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale);
    return g_launches;
}
