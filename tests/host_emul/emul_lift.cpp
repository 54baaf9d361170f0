// csrc/k_lift.hip compiled for the host (tests/test_lift_host_cpu.py).
#include "kernels.h"
#include "k_lift.hip"
extern "C" {
void emul_lift_windows(const float* track, int P, int64_t n, float width, float height, int T, int stride, const int* resample, int flip, float* x) {
    kasf_launch_lift_windows(nullptr, track, P, n, width, height, T, stride, resample, flip, x);
}
void emul_lift_stitch(const float* pred, int flip, int P, int64_t n, int T, int stride, const int* first_pos, float* out) {
    kasf_launch_lift_stitch(nullptr, pred, flip, P, n, T, stride, first_pos, out);
}
void emul_lift_windows_ragged(const float* track, int64_t frames, const int64_t* offsets, const int64_t* win_first, int P, int64_t windows, const float* width,
                              const float* height, int T, int stride, const int* resample, int flip, float* x) {
    kasf_launch_lift_windows_ragged(nullptr, track, frames, offsets, win_first, P, windows, width, height, T, stride, resample, flip, x);
}
void emul_lift_stitch_ragged(const float* pred, int flip, int64_t windows, const int64_t* offsets, const int64_t* win_first, int P, int64_t frames, int T,
                             int stride, const int* first_pos, float* out) {
    kasf_launch_lift_stitch_ragged(nullptr, pred, flip, windows, offsets, win_first, P, frames, T, stride, first_pos, out);
}
void emul_stream_push(const float* frames, const int* slots, int K, int S, int T, float* ring, int64_t* count) {
    kasf_launch_stream_push(nullptr, frames, slots, K, S, T, ring, count);
}
void emul_stream_windows(const float* ring, const int64_t* count, const int* slots, int K, int S, int T, const float* width, const float* height,
                         const int* resample_tab, int flip, float* x) {
    kasf_launch_stream_windows(nullptr, ring, count, slots, K, S, T, width, height, resample_tab, flip, x);
}
void emul_stream_emit(const float* pred, int flip, const int64_t* count, const int* slots, int K, int S, int T, const int* first_pos_tab, int back, int n_out,
                      float* out) {
    kasf_launch_stream_emit(nullptr, pred, flip, count, slots, K, S, T, first_pos_tab, back, n_out, out);
}
}
