// csrc/k_stream_track.hip compiled for the host (tests/test_tracked_host_cpu.py).
#include "kernels.h"
#include "k_stream_track.hip"
extern "C" void emul_front(const float* frames, const int* ids, const int* slot, const int* born, const int* count_b, int B, int S_t, int rows_mode, int R, int T,
                           float* ring, int64_t* count, int* owner, const float* width, const float* height, const int* resample_tab, int flip, float* x,
                           int* row_slot) {
    kasf_launch_stream_track_front(nullptr, frames, ids, slot, born, count_b, B, S_t, rows_mode, R, T, ring, count, owner, width, height, resample_tab, flip, x, row_slot);
}
extern "C" void emul_emit(const float* pred, int flip, const int64_t* count, const int* owner, const int* row_slot, int64_t n_rows, int T, const int* first_pos_tab,
                          int back, float* out, unsigned char* valid, int* ids_out, int64_t* frames_out) {
    kasf_launch_stream_track_emit(nullptr, pred, flip, count, owner, row_slot, n_rows, T, first_pos_tab, back, out, valid, ids_out, frames_out);
}
