// Decoder surfaces -> BGR frames (kasf.h, kasf_yuv420_to_bgr): the YUV 4:2:0 -> BGR conversion that stands behind the demo's cap.read(), from the NV12 surface a
// hardware decoder leaves in device memory (or a software decoder's planar I420) to the uint8 [Hf][Wf][3] frame k_letterbox.hip and k_crop.hip read.
// One launch; no atomics, no scratch, no LDS, nothing that depends on n_frames.  Pure bandwidth: 1.5 bytes read and 3 written per pixel.
// MAPPING.  As k_letterbox.hip: a workgroup of 256 threads serves one frame (blockIdx.y, strided past 65,535) and walks chunks of 256 items.  An item is
//   a BLOCK of 2 rows x 8 columns (the vector form): the four chroma samples are loaded once for both rows -- one 8-byte load of the NV12 pairs, or one dword
//     each of the I420 planes --, each row's eight luma samples are one 8-byte load, and each row's 24 output bytes leave as six whole dwords.  Consecutive
//     lanes own consecutive blocks of a row pair, so a wavefront's luma load covers 512 consecutive bytes and its stores 1,536.
//   a QUAD of 2 x 2 pixels around one chroma sample (the element form), read and written byte by byte with each pixel checked against Hf and Wf.
// Pointers and pitches are bytes with no alignment promised (kasf.h, rule 1).  The launch takes the vector form for the Wf / 8 x Hf / 2 whole blocks only when
// every base pointer and stride it uses is aligned to its access -- 8 bytes for the luma plane and the NV12 chroma plane, 4 for the I420 chroma planes and the
// output --; quads cover the rest: the columns right of the last whole block, the last row of an odd Hf, and everything when something is unaligned, Wf < 8 or
// Hf < 2.  Blocks come first in a frame's item order, then the right strip's quads, then the bottom row's: one kernel, divergent in at most one wavefront per
// boundary.
// ARITHMETIC (rule 3).  Per chroma sample the three chroma sums with the rounding constant folded in, per pixel one multiply for the luma, three adds, three
// shifts and clamps: integer sums are exact, so this grouping gives rule 3's bits.  Every product has operands below 2^23 (coefficients < 2,215,015, samples
// <= 255), so they are the full-rate 24-bit multiplies.
#include "kernels.h"

namespace {

constexpr int YUV_THREADS = 256;

struct YuvCoef { int cy, cvr, cvg, cug, cub, yoff; };             // rule 4's table; yoff = 16 (limited range) or 0

struct alignas(8) Bytes8 { unsigned e[2]; };
struct alignas(4) Bytes24 { unsigned e[6]; };

__device__ inline int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

struct ChromaTerms { int r, g, b; };
__device__ inline ChromaTerms chroma_terms(int U, int V, const YuvCoef& k) {
    const int u = U - 128, v = V - 128;
    ChromaTerms t;
    t.r = __mul24(k.cvr, v) + (1 << 19);
    t.g = __mul24(k.cvg, v) + __mul24(k.cug, u) + (1 << 19);
    t.b = __mul24(k.cub, u) + (1 << 19);
    return t;
}
// one pixel -> its three output bytes in output order (rule 5)
__device__ inline void pixel(int Y, const ChromaTerms& t, const YuvCoef& k, int rgb, int c[3]) {
    int y = Y - k.yoff;
    y = y < 0 ? 0 : y;
    const int y1 = __mul24(y, k.cy);
    const int R = sat8((y1 + t.r) >> 20), G = sat8((y1 + t.g) >> 20), B = sat8((y1 + t.b) >> 20);
    c[0] = rgb ? R : B;
    c[1] = G;
    c[2] = rgb ? B : R;
}

template <bool NV12>
__global__ __launch_bounds__(YUV_THREADS) void k_yuv420_to_bgr(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ c0,
                                                               const unsigned char* __restrict__ c1, int n_frames, int Hf, int Wf, int64_t y_rs, int64_t c_rs,
                                                               int64_t y_fs, int64_t c_fs, unsigned char* __restrict__ out, int64_t o_rs, int64_t o_fs, YuvCoef k,
                                                               int rgb, int bw, int bh) {         // bw x bh whole blocks in the vector form (0 x 0: none)
    const int tid = threadIdx.x;
    const int cw = (Wf + 1) >> 1, ch = (Hf + 1) >> 1;
    const int qx0 = 4 * bw;                                    // first quad column right of the blocks
    const int n_vec = bw * bh;                                 // <= 4,095 * 16,383
    const int wA = cw - qx0, nA = wA * ch;                     // the right strip: every chroma row
    const int nB = (ch - bh) * qx0;                            // the bottom row of an odd Hf, under the blocks
    const int items = n_vec + nA + nB;                         // <= cw * ch <= 2^28
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const unsigned char* __restrict__ fy = yp + f * y_fs;
        const unsigned char* __restrict__ fc0 = c0 + f * c_fs;
        const unsigned char* __restrict__ fc1 = NV12 ? nullptr : c1 + f * c_fs;
        unsigned char* __restrict__ fo = out + f * o_fs;
        for (int i = blockIdx.x * YUV_THREADS + tid; i < items; i += gridDim.x * YUV_THREADS) {
            if (i < n_vec) {                                   // rows 2 by, 2 by + 1, columns 8 bx .. 8 bx + 7: inside the frame by the choice of bw, bh
                const int by = i / bw, bx = i - by * bw;
                const int x = 8 * bx;
                const unsigned char* __restrict__ row = fy + (int64_t)(2 * by) * y_rs + x;
                const Bytes8 ya = *reinterpret_cast<const Bytes8*>(row), yb = *reinterpret_cast<const Bytes8*>(row + y_rs);
                int U[4], V[4];
                if (NV12) {
                    const Bytes8 uv = *reinterpret_cast<const Bytes8*>(fc0 + (int64_t)by * c_rs + x);          // U0 V0 U1 V1 | U2 V2 U3 V3
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        U[j] = (int)((uv.e[j >> 1] >> (16 * (j & 1))) & 255u);
                        V[j] = (int)((uv.e[j >> 1] >> (16 * (j & 1) + 8)) & 255u);
                    }
                } else {
                    const unsigned uu = *reinterpret_cast<const unsigned*>(fc0 + (int64_t)by * c_rs + (x >> 1));
                    const unsigned vv = *reinterpret_cast<const unsigned*>(fc1 + (int64_t)by * c_rs + (x >> 1));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        U[j] = (int)((uu >> (8 * j)) & 255u);
                        V[j] = (int)((vv >> (8 * j)) & 255u);
                    }
                }
                Bytes24 oa, ob;
#pragma unroll
                for (int q = 0; q < 6; ++q) oa.e[q] = ob.e[q] = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const ChromaTerms t = chroma_terms(U[j], V[j], k);
#pragma unroll
                    for (int d = 0; d < 2; ++d) {
                        const int p = 2 * j + d;                                                              // the pixel's column in the block
                        int ca[3], cb[3];
                        pixel((int)((ya.e[p >> 2] >> (8 * (p & 3))) & 255u), t, k, rgb, ca);
                        pixel((int)((yb.e[p >> 2] >> (8 * (p & 3))) & 255u), t, k, rgb, cb);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int b = 3 * p + c;                                                          // the byte's place in the row's 24
                            oa.e[b >> 2] |= (unsigned)ca[c] << (8 * (b & 3));
                            ob.e[b >> 2] |= (unsigned)cb[c] << (8 * (b & 3));
                        }
                    }
                }
                unsigned char* __restrict__ o = fo + (int64_t)(2 * by) * o_rs + 3 * x;
                *reinterpret_cast<Bytes24*>(o) = oa;
                *reinterpret_cast<Bytes24*>(o + o_rs) = ob;
            } else {                                           // one chroma sample and the up to four pixels that share it
                int r = i - n_vec, qy, qx;
                if (r < nA) {
                    qy = r / wA;
                    qx = qx0 + (r - qy * wA);
                } else {
                    r -= nA;
                    const int q = r / qx0;
                    qy = bh + q;
                    qx = r - q * qx0;
                }
                const int64_t coff = (int64_t)qy * c_rs;
                const int U = NV12 ? fc0[coff + 2 * qx] : fc0[coff + qx];
                const int V = NV12 ? fc0[coff + 2 * qx + 1] : fc1[coff + qx];
                const ChromaTerms t = chroma_terms(U, V, k);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int y = 2 * qy + dy, x = 2 * qx + dx;
                        if (y < Hf && x < Wf) {
                            int c[3];
                            pixel(fy[(int64_t)y * y_rs + x], t, k, rgb, c);
                            unsigned char* __restrict__ o = fo + (int64_t)y * o_rs + 3 * x;
                            o[0] = (unsigned char)c[0];
                            o[1] = (unsigned char)c[1];
                            o[2] = (unsigned char)c[2];
                        }
                    }
            }
        }
    }
}

inline bool on_grid(const void* p, int64_t a, int64_t b, int n) { return (((uintptr_t)p | (uintptr_t)a | (uintptr_t)b) & (uintptr_t)(n - 1)) == 0; }

}  // namespace

void kasf_launch_yuv420_to_bgr(hipStream_t s, const void* y, const void* c0, const void* c1, int nv12, int n_frames, int Hf, int Wf, int64_t y_row_stride,
                               int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride, void* out, int64_t out_row_stride, int64_t out_frame_stride,
                               const int coef[5], int full_range, int rgb) {
    if (n_frames <= 0) return;
    if (n_frames == 1) y_frame_stride = c_frame_stride = out_frame_stride = 0;      // never used: no alignment to ask of them
    const bool vec = Wf >= 8 && Hf >= 2 && on_grid(y, y_row_stride, y_frame_stride, 8) && on_grid(out, out_row_stride, out_frame_stride, 4) &&
                     (nv12 ? on_grid(c0, c_row_stride, c_frame_stride, 8) : on_grid(c0, c_row_stride, c_frame_stride, 4) && on_grid(c1, 0, 0, 4));
    const int bw = vec ? Wf / 8 : 0, bh = vec ? Hf / 2 : 0;
    const int cw = (Wf + 1) / 2, ch = (Hf + 1) / 2;
    const int64_t items = (int64_t)bw * bh + (int64_t)(cw - 4 * bw) * ch + (int64_t)(ch - bh) * 4 * bw;
    int64_t bpf = (items + YUV_THREADS - 1) / YUV_THREADS;              // workgroups per frame: one chunk each while that keeps the launch under ~8 per CU,
    if (n_frames * bpf > 2048) bpf = (bpf + 3) / 4;                     // four chunks each beyond
    const dim3 grid((unsigned)bpf, (unsigned)(n_frames > 65535 ? 65535 : n_frames)), block(YUV_THREADS);
    const YuvCoef k = {coef[0], coef[1], coef[2], coef[3], coef[4], full_range ? 0 : 16};
    const unsigned char *yp = (const unsigned char*)y, *p0 = (const unsigned char*)c0, *p1 = (const unsigned char*)c1;
#define KASF_YUV_LAUNCH(NV)                                                                                                                          \
    hipLaunchKernelGGL((k_yuv420_to_bgr<NV>), grid, block, 0, s, yp, p0, p1, n_frames, Hf, Wf, y_row_stride, c_row_stride, y_frame_stride, c_frame_stride, \
                       (unsigned char*)out, out_row_stride, out_frame_stride, k, rgb, bw, bh)
    if (nv12) KASF_YUV_LAUNCH(true); else KASF_YUV_LAUNCH(false);
#undef KASF_YUV_LAUNCH
}
