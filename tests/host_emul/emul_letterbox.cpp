// csrc/k_letterbox.hip compiled for the host (tests/test_letterbox_host_cpu.py).
#include "kernels.h"
#include "k_letterbox.hip"
extern "C" int emul_letterbox(const void* frames, int n_frames, int Hf, int Wf, int64_t row_stride, int64_t frame_stride, void* out, int out_dtype, int out_w,
                              int out_h, int new_w, int new_h, int pad_x, int pad_y, int pad_value, int swap_rb) {
    g_lds_overrun = 0;
    kasf_launch_letterbox(nullptr, frames, n_frames, Hf, Wf, row_stride, frame_stride, out, out_dtype, out_w, out_h, new_w, new_h, pad_x, pad_y, pad_value, swap_rb);
    return g_lds_overrun;                              // 1: a workgroup wrote past the dynamic LDS it asked for
}
