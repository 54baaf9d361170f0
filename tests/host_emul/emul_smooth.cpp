// csrc/k_smooth.hip compiled for the host (tests/test_smooth_host_cpu.py).  p: dt, min_cutoff, d_cutoff, beta, min_score.
#include "kernels.h"
#include "k_smooth.hip"
static KasfOneEuro params_of(const float* p, int max_hold) { return KasfOneEuro{p[0], p[1], p[2], p[3], p[4], max_hold}; }
extern "C" void emul_push(const float* x, const int* slots, int K, int S, int J, int C, int has_score, const float* p, int max_hold, int64_t tick, float* xhat,
                          float* dxhat, int64_t* last, float* out) {
    kasf_launch_one_euro_push(nullptr, x, slots, K, S, J, C, has_score, params_of(p, max_hold), tick, xhat, dxhat, last, out);
}
extern "C" void emul_tracked(const float* x, const int* ids, const int* slot, const int* born, const int* count_b, int B, int S_t, int rows_mode, int R, int J, int C,
                             int has_score, const float* p, int max_hold, int64_t tick, float* xhat, float* dxhat, int64_t* last, int* owner, float* out,
                             int* row_slot) {
    kasf_launch_one_euro_tracked(nullptr, x, ids, slot, born, count_b, B, S_t, rows_mode, R, J, C, has_score, params_of(p, max_hold), tick, xhat, dxhat, last, owner,
                                 out, row_slot);
}
extern "C" void emul_tracks(const float* x, const int64_t* offsets, int64_t N, int P, int J, int C, int has_score, const float* p, int max_hold, float* out) {
    kasf_launch_one_euro_tracks(nullptr, x, offsets, N, P, J, C, has_score, params_of(p, max_hold), out);
}
