// csrc/k_yuv.hip compiled for the host (tests/test_yuv_host_cpu.py).
#include "kernels.h"
#include "k_yuv.hip"
// -> the number of launches made (the entry point promises one), or -1 if one of them asked for LDS
extern "C" int emul_yuv420_to_bgr(const void* y, const void* c0, const void* c1, int nv12, int n_frames, int Hf, int Wf, int64_t y_row_stride, int64_t c_row_stride,
                                  int64_t y_frame_stride, int64_t c_frame_stride, void* out, int64_t out_row_stride, int64_t out_frame_stride, const int* coef,
                                  int full_range, int rgb) {
    g_lds_asked = g_launches = 0;
    kasf_launch_yuv420_to_bgr(nullptr, y, c0, c1, nv12, n_frames, Hf, Wf, y_row_stride, c_row_stride, y_frame_stride, c_frame_stride, out, out_row_stride,
                              out_frame_stride, coef, full_range, rgb);
    return g_lds_asked ? -1 : g_launches;
}
