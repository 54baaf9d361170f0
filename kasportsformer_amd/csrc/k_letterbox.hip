// Video frames -> detector inputs (kasf.h, kasf_letterbox_frames): what the demo's prep_image does on the host in front of YOLOv3
//   letterbox_image: cv2.resize(INTER_CUBIC) onto a canvas of 128   demo/lib/yolov3/preprocess.py:9-21, restated as the fixed-point scheme of OpenCV's portable
//                                                                    8-bit path: 11-bit coefficients, integer sums, a 22-bit rounding shift (kasf.h, rules 2-3)
//   [:, :, ::-1], transpose, float().div(255.0)                     preprocess.py:36-37 (rule 4: a table of the 256 possible outputs, planes stored swapped)
// One launch that writes every output element, padding included; no atomics, no scratch, nothing that depends on n_frames.
// MAPPING.  As k_crop.hip: a workgroup of 256 threads serves one frame (blockIdx.y, strided past 65,535) and walks chunks of 256 "groups"; a group is PX = 4
// consecutive pixels of one output row, so each of a thread's three planes leaves in ONE store of 16 bytes (fp32) or 8 bytes (fp16 / bf16) and a wavefront's
// store instruction covers 1 KiB / 512 B of consecutive addresses.  (Eight 16-bit pixels per group, a 16-byte store, was measured and dropped: 16 frames of
// 1080p -> 416 took 55 us in fp16 against 32 us in fp32 -- half the threads, each with twice the dependent work -- and take 31 us with four.)  Widths that
// are no multiple of 4, or a base that is not aligned to the store, take the same kernel with PX = 1.  Padding groups take the same store path with the pad
// value in every lane.
// TABLES.  Per workgroup, once, in dynamic LDS: the column table (x0, w[0..3]: rule 2's sx and a[0..3] with the clamp folded in, see TAPS) for the new_w columns of the resized image (12 bytes each: one fp64
// multiply and about thirty fp32 operations per column instead of per tap) and the 256 possible outputs of rule 4, already in the output type.  The row's
// (sy, b[0..3]) are formed once per thread and group, i.e. once per PX pixels x 16 taps x 3 channels.
// TAPS.  A direct 16-tap gather: when 1080p shrinks to 416 neighbouring output pixels share no source pixels, so a two-pass tile would reuse nothing.  The four
// clamped taps of a column always lie inside one window of four pixels, x0 = clamp(sx - 1, 0, Wf - 4) onwards; taps that the clamp sends to the same pixel
// have their weights added in the table (rule 3's sum regrouped: integers, so the same V).  So the inner loop has no edge case and no divergent branch: per
// source row one 12-byte read (three unaligned dwords) at rows[ky] + 3 x0, always inside the row.  Only a frame of fewer than four columns reads byte by byte
// (a launch-uniform branch).  All sums are int32 (|V| < 2^31, kasf.h) and every product has operands of at most 21 bits (weights of 13, a row sum below
// 255 * 1.376 * 2048 < 2^20), so they are the full-rate 24-bit multiplies; a 1080p frame (6 MB) stays in L2.
#include "kernels.h"

namespace {

constexpr int LB_THREADS = 256;

template <class T> __device__ inline T lb_out(float f);
template <> __device__ inline float lb_out<float>(float f) { return f; }
template <> __device__ inline _Float16 lb_out<_Float16>(float f) { return (_Float16)f; }      // round to nearest even
template <> __device__ inline __bf16 lb_out<__bf16>(float f) { return (__bf16)f; }            // round to nearest even

// rule 2 for one axis: position d of the resized image -> s = floorf(fx) and the four 11-bit weights of taps s - 1 .. s + 2
__device__ inline void cubic_taps(int d, double scale, int& s, int a[4]) {
    const float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    const float t = f - fl;
    const float A = -0.75f;
    const float u = t + 1.0f, w = 1.0f - t;
    float c[4];
    c[0] = ((A * u - 5 * A) * u + 8 * A) * u - 4 * A;
    c[1] = ((A + 2) * t - (A + 3)) * t * t + 1;
    c[2] = ((A + 2) * w - (A + 3)) * w * w + 1;
    c[3] = 1.0f - c[0] - c[1] - c[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = (int)rintf(c[k] * 2048.0f);      // half to even
    s = (int)fl;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <class T, int PX, bool WIDE>                          // WIDE: Wf >= 4, a window of four pixels fits a row
__global__ __launch_bounds__(LB_THREADS) void k_letterbox(const unsigned char* __restrict__ frames, int n_frames, int Hf, int Wf, int64_t row_stride,
                                                          int64_t frame_stride, T* __restrict__ out, int out_w, int out_h, int new_w, int new_h, int pad_x,
                                                          int pad_y, double scale_x, double scale_y, int pad_value, int swap_rb) {
    HIP_DYNAMIC_SHARED(int, lds)                                // [new_w][3] ints = x0, w0 | w1 << 16, w2 | w3 << 16; then T table[256]
    int* __restrict__ cols = lds;
    T* __restrict__ table = reinterpret_cast<T*>(lds + 3 * new_w);
    const int tid = threadIdx.x;
    // (the two table loops stay scalar: vectorised by two they become packed fp32 with operand select, which tests/test_packed_fp32_guard_cpu.py keeps out)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int e = tid; e < 256; e += LB_THREADS) table[e] = lb_out<T>((float)e / 255.0f);      // rule 4, for every value a channel can take
#pragma clang loop vectorize(disable) interleave(disable)
    for (int dx = tid; dx < new_w; dx += LB_THREADS) {
        int s, a[4];
        cubic_taps(dx, scale_x, s, a);
        // rule 3's clamped taps all lie in the window of pixels x0 .. x0 + 3: taps that clamp to one pixel add their weights (integers: the same sum)
        const int x0 = clampi(s - 1, 0, WIDE ? Wf - 4 : 0);
        int w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = clampi(s - 1 + k, 0, Wf - 1) - x0;     // 0 .. 3
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] += i == q ? a[k] : 0;
        }
        cols[3 * dx] = x0;
        cols[3 * dx + 1] = (int)(((unsigned)w[0] & 0xffffu) | ((unsigned)w[1] << 16));
        cols[3 * dx + 2] = (int)(((unsigned)w[2] & 0xffffu) | ((unsigned)w[3] << 16));
    }
    __syncthreads();
    const int gpr = (out_w + PX - 1) / PX;                      // groups per row
    const int groups = gpr * out_h;                             // <= 2^24 (out_w, out_h <= 4096)
    const int64_t plane = (int64_t)out_h * out_w;
    const T padv = table[pad_value];
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const unsigned char* __restrict__ frame = frames + f * frame_stride;
        T* __restrict__ op = out + f * 3 * plane;
        for (int g = blockIdx.x * LB_THREADS + tid; g < groups; g += gridDim.x * LB_THREADS) {
            const int y = g / gpr, x0 = (g - y * gpr) * PX;
            const int dy = y - pad_y;
            T val[3][PX];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < PX; ++j) val[c][j] = padv;
            if ((unsigned)dy < (unsigned)new_h) {               // rule 1: a row of the resized image
                int sy, b[4];
                cubic_taps(dy, scale_y, sy, b);
                const unsigned char* __restrict__ rows[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) rows[k] = frame + (int64_t)clampi(sy - 1 + k, 0, Hf - 1) * row_stride;
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    const int dx = x0 + j - pad_x;
                    const bool image = (unsigned)dx < (unsigned)new_w;                           // otherwise a padding column: computed on column 0, not kept
                    const int e = 3 * (image ? dx : 0);
                    const int off = 3 * cols[e], w01 = cols[e + 1], w23 = cols[e + 2];
                    const int w[4] = {(int)((unsigned)w01 << 16) >> 16, w01 >> 16, (int)((unsigned)w23 << 16) >> 16, w23 >> 16};
                    int V[3] = {0, 0, 0};
#pragma unroll
                    for (int ky = 0; ky < 4; ++ky) {
                        const unsigned char* __restrict__ src = rows[ky] + off;
                        int p[12];
                        if (WIDE) {                                                              // bytes 3 x0 .. 3 x0 + 11 of the row: inside it (x0 <= Wf - 4)
                            unsigned d[3];
                            __builtin_memcpy(d, src, 12);
#pragma unroll
                            for (int i = 0; i < 12; ++i) p[i] = (int)((d[i >> 2] >> (8 * (i & 3))) & 255u);
                        } else {                                                                 // a frame of one to three columns: x0 = 0, what lies past the row weighs 0
#pragma unroll
                            for (int i = 0; i < 12; ++i) p[i] = src[i < 3 * Wf ? i : 0];
                        }
#pragma unroll
                        for (int c = 0; c < 3; ++c)                                              // 24-bit operands: |w|, |b| < 2^12, p <= 255, |row sum| < 2^20
                            V[c] += __mul24(b[ky], __mul24(w[0], p[c]) + __mul24(w[1], p[3 + c]) + __mul24(w[2], p[6 + c]) + __mul24(w[3], p[9 + c]));
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const T v = table[clampi((V[c] + (1 << 21)) >> 22, 0, 255)];               // rule 3
                        val[c][j] = image ? v : padv;
                    }
                }
            }
            T* __restrict__ o = op + (int64_t)y * out_w + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                T* __restrict__ dst = o + (swap_rb ? 2 - c : c) * plane;                       // rule 4: plane k holds frame channel 2 - k
                if (PX == 1) {
                    dst[0] = val[c][0];
                } else {
                    struct alignas(PX * sizeof(T)) Vec { T e[PX]; };
                    Vec v;
#pragma unroll
                    for (int j = 0; j < PX; ++j) v.e[j] = val[c][j];
                    *reinterpret_cast<Vec*>(dst) = v;
                }
            }
        }
    }
}

template <class T>
void launch(hipStream_t s, const unsigned char* frames, int n_frames, int Hf, int Wf, int64_t row_stride, int64_t frame_stride, void* out, int out_w, int out_h,
            int new_w, int new_h, int pad_x, int pad_y, int pad_value, int swap_rb) {
    constexpr int VPX = 4, VBYTES = VPX * (int)sizeof(T);
    const bool vec = ((uintptr_t)out & (VBYTES - 1)) == 0 && out_w % VPX == 0;    // then every row of every plane of every frame starts on such a boundary
    const int px = vec ? VPX : 1;
    const int64_t groups = (int64_t)((out_w + px - 1) / px) * out_h;
    int64_t bpf = (groups + LB_THREADS - 1) / LB_THREADS;               // workgroups per frame: one chunk each while that keeps the launch under ~8 per CU,
    if (n_frames * bpf > 2048) bpf = (bpf + 3) / 4;                     // four chunks each beyond (the tables are formed once per workgroup)
    const double scale_x = 1.0 / ((double)new_w / (double)Wf), scale_y = 1.0 / ((double)new_h / (double)Hf);       // rule 2: two roundings each
    const dim3 grid((unsigned)bpf, (unsigned)(n_frames > 65535 ? 65535 : n_frames)), block(LB_THREADS);
    const size_t lds = (size_t)new_w * 12 + 256 * sizeof(T);            // <= 49 KiB (new_w <= 4096)
#define KASF_LB_LAUNCH(PXV, WIDEV)                                                                                                                      \
    hipLaunchKernelGGL((k_letterbox<T, PXV, WIDEV>), grid, block, lds, s, frames, n_frames, Hf, Wf, row_stride, frame_stride, (T*)out, out_w, out_h, new_w, \
                       new_h, pad_x, pad_y, scale_x, scale_y, pad_value, swap_rb)
    if (Wf >= 4) {
        if (vec) KASF_LB_LAUNCH(VPX, true); else KASF_LB_LAUNCH(1, true);
    } else {
        if (vec) KASF_LB_LAUNCH(VPX, false); else KASF_LB_LAUNCH(1, false);
    }
#undef KASF_LB_LAUNCH
}

}  // namespace

void kasf_launch_letterbox(hipStream_t s, const void* frames, int n_frames, int Hf, int Wf, int64_t row_stride, int64_t frame_stride, void* out, int out_dtype,
                           int out_w, int out_h, int new_w, int new_h, int pad_x, int pad_y, int pad_value, int swap_rb) {
    if (n_frames <= 0) return;
    const unsigned char* f = (const unsigned char*)frames;
    if (out_dtype == KASF_F32)
        launch<float>(s, f, n_frames, Hf, Wf, row_stride, frame_stride, out, out_w, out_h, new_w, new_h, pad_x, pad_y, pad_value, swap_rb);
    else if (out_dtype == KASF_F16)
        launch<_Float16>(s, f, n_frames, Hf, Wf, row_stride, frame_stride, out, out_w, out_h, new_w, new_h, pad_x, pad_y, pad_value, swap_rb);
    else
        launch<__bf16>(s, f, n_frames, Hf, Wf, row_stride, frame_stride, out, out_w, out_h, new_w, new_h, pad_x, pad_y, pad_value, swap_rb);
}
