// Tracked skeletons -> the frame and the encoder's surface (kasf.h, kasf_draw_poses / kasf_bgr_to_nv12 / kasf_pose_panel): what the demo's plot_on_frame and
// cv2.VideoWriter do on the host (demo/demo.py:91-105, 307-323), as one launch that paints opaque lines, dots and filled rectangles over the uint8 BGR frame
// and writes the painted frame and / or its NV12 surface.  All geometry is in integers (rules 1-3); no atomics, no scratch.
// MAPPING.  A workgroup of 256 threads owns a TILE of 128 columns x 32 rows of one frame (blockIdx.x: the tile, blockIdx.y: the frame, strided past 65,535).
//   A thread owns a BLOCK of 2 rows x 8 columns = four whole 2 x 2 quads, sixteen packed pixels in registers: it reads them, paints them, forms their luma and
//   its four chroma samples itself and writes all of it, so nothing is shared between threads and out_bgr == frames is safe.  Consecutive lanes own consecutive
//   blocks of a row pair (16 across, 16 down), so a wavefront's row is 384 consecutive bytes of the frame and 128 of the luma plane.
// BINNING.  The frame's primitives in rule 2's order are fills 0..R-1, then per person and segment: line, dot, dot -- N = R + 3 S P of them, addressed by index
//   alone.  The workgroup walks them in chunks of DRAW_LIST = 256 from the LAST to the first: thread t decodes primitive base + t (visibility by rule 1, then an
//   exact, conservative bounding box -- the segment's box grown by ceil(t / 2), the dot's by r, the clipped rectangle -- against the tile), the hits are
//   compacted IN ORDER into the LDS list (one __ballot per wavefront, the four counts through LDS), and every thread walks the list backwards over the pixels it
//   has not painted yet: the first hit is the last primitive that covers the pixel.  The per-pixel "painted" bits carry over to the next (earlier) chunk, so a
//   tile that any number of primitives touch is right; a chunk's list cannot overflow because it has as many entries as the chunk has primitives.
//   With N = 0 (kasf_bgr_to_nv12) the loop and its barriers are never entered.
// FORMS.  Each of the four streams (frame in, frame out, luma, chroma) moves a whole block as dwords where its base pointer and strides are aligned (4 bytes for
//   the frames, 8 for the planes) and the block lies inside the frame, byte by byte with every pixel checked against Hf and Wf otherwise -- chosen per stream by
//   the launch, per block by the kernel, as k_yuv.hip chooses.  In place, a block that nothing painted is not stored again (the bytes are already there).
// ARITHMETIC.  Rule 3 without a wide multiplication per pixel: the thread that decodes a line forms K = isqrt(floor(t^2 L2 / 4)) once, so that between the ends
//   4 c^2 <= t^2 L2 is |c| <= K; at the ends 4 (u . u) <= t^2 is u . u <= floor(t^2 / 4) on operands within 32.  s = w . d and c = w x d are formed in int64 once
//   per (block, line) and stepped per pixel by additions.  The same bits as the rule (kasf.h allows any arrangement that gives them); rule 5's sums are int32.
#include "kernels.h"

namespace {

constexpr int DRAW_THREADS = 256;
constexpr int DRAW_BLOCK_W = 8, DRAW_BLOCK_H = 2;                 // a thread's pixels
constexpr int DRAW_TILE_W = 16 * DRAW_BLOCK_W, DRAW_TILE_H = 16 * DRAW_BLOCK_H;      // 128 x 32
constexpr int DRAW_LIST = 256;                                    // primitives per chunk = entries of the LDS list
constexpr unsigned KIND_FILL = 0u, KIND_LINE = 1u, KIND_DOT = 2u;

struct DrawArgs {
    const unsigned char* frames; int64_t f_rs, f_fs;
    unsigned char* out; int64_t o_rs, o_fs;
    unsigned char *oy, *ouv; int64_t y_rs, uv_rs, y_fs, uv_fs;
    const float* kp; int64_t kp_f, kp_p, kp_j, kp_c;
    const unsigned char* valid; int64_t v_f, v_p;
    const int* seg; const unsigned char* col; const int* fills;
    int n_frames, Hf, Wf, P, J, S, R, t, r, use_score;
    float min_score;
    unsigned dot;                                                 // dot_color, packed as a pixel
    int ky[3], ku[3], kv[3], yoff;                                // rule 5's coefficients by the frame's channel position
    int vec_in, vec_out, vec_y, vec_uv, in_place;
};

struct alignas(8) DBytes8 { unsigned e[2]; };
struct alignas(4) DBytes24 { unsigned e[6]; };

__device__ inline int dsat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// rule 1: joint j of person p -> its pixel, or false
__device__ inline bool draw_joint(const DrawArgs& a, int64_t f, int p, int j, int& xi, int& yi) {
    if (j < 0 || j >= a.J) return false;
    const float* q = a.kp + f * a.kp_f + (int64_t)p * a.kp_p + (int64_t)j * a.kp_j;
    const float x = q[0], y = q[a.kp_c];
    if (!(fabsf(x) < 1.0e6f) || !(fabsf(y) < 1.0e6f)) return false;               // NaN, inf and everything far outside rule 1's bounds: the casts below are defined
    xi = (int)x;
    yi = (int)y;
    if (xi < -32768 || xi > 65535 || yi < -32768 || yi > 65535) return false;
    if (a.use_score && !(q[2 * a.kp_c] > a.min_score)) return false;
    return true;
}

// rule 3's threshold between the ends, once per line: 4 c^2 <= t^2 L2  <=>  c^2 <= floor(t^2 L2 / 4)  <=>  |c| <= K = isqrt(floor(t^2 L2 / 4)), K < 2^23.
// The double square root only has to land near K: the two loops make it exact (M < 2^47, so every product below fits int64).
__device__ inline int draw_line_reach(int dx, int dy, int t) {
    const int64_t L2 = (int64_t)dx * dx + (int64_t)dy * dy, M = ((int64_t)t * t * L2) >> 2;
    int64_t k = (int64_t)sqrt((double)M);
    while (k * k > M) --k;
    while ((k + 1) * (k + 1) <= M) ++k;
    return (int)k;
}

// primitive i of frame f in rule 2's order -> its list entry, if it is drawn and its bounding box meets the tile [tx0, tx1) x [ty0, ty1)
__device__ inline bool draw_decode(const DrawArgs& a, int64_t f, int i, int tx0, int ty0, int tx1, int ty1, int& ax, int& ay, int& bx, int& by, unsigned& kc, int& reach) {
    int lox, loy, hix, hiy;                                       // the box, inclusive
    if (i < a.R) {
        const int* q = a.fills + 7 * (int64_t)i;
        ax = q[0] < 0 ? 0 : q[0];
        ay = q[1] < 0 ? 0 : q[1];
        bx = q[2] > a.Wf ? a.Wf : q[2];
        by = q[3] > a.Hf ? a.Hf : q[3];
        if (ax >= bx || ay >= by) return false;
        kc = (KIND_FILL << 24) | (unsigned)(q[4] & 255) | ((unsigned)(q[5] & 255) << 8) | ((unsigned)(q[6] & 255) << 16);
        lox = ax; loy = ay; hix = bx - 1; hiy = by - 1;
    } else {
        const int k = i - a.R, per = 3 * a.S;
        const int p = k / per, m = k - p * per, s = m / 3, which = m - 3 * s;
        if (a.valid && a.valid[f * a.v_f + (int64_t)p * a.v_p] == 0) return false;
        const int ja = a.seg[2 * s], jb = a.seg[2 * s + 1];
        if (which == 0) {
            if (!draw_joint(a, f, p, ja, ax, ay) || !draw_joint(a, f, p, jb, bx, by)) return false;
            const unsigned char* c = a.col + 3 * s;
            kc = (KIND_LINE << 24) | (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
            const int h = (a.t + 1) >> 1;
            lox = (ax < bx ? ax : bx) - h; hix = (ax < bx ? bx : ax) + h;
            loy = (ay < by ? ay : by) - h; hiy = (ay < by ? by : ay) + h;
            if (!(lox < tx1 && hix >= tx0 && loy < ty1 && hiy >= ty0)) return false;
            reach = draw_line_reach(bx - ax, by - ay, a.t);
            return true;
        } else {
            if (!draw_joint(a, f, p, which == 1 ? ja : jb, ax, ay)) return false;
            bx = ax; by = ay;
            kc = (KIND_DOT << 24) | a.dot;
            lox = ax - a.r; hix = ax + a.r; loy = ay - a.r; hiy = ay + a.r;
        }
    }
    return lox < tx1 && hix >= tx0 && loy < ty1 && hiy >= ty0;
}

// rule 3 at an end: 4 (u . u) <= t^2  <=>  u . u <= E = floor(t^2 / 4) <= 1024, which needs |ux|, |uy| <= 32: small squares
__device__ inline bool draw_near(int ux, int uy, int E) { return ux >= -32 && ux <= 32 && uy >= -32 && uy <= 32 && ux * ux + uy * uy <= E; }

// rule 3, one pixel against line A -> B: w = pixel - A, s = w . d, c = w x d -- no multiplication wider than 32 bits per pixel
__device__ inline bool draw_on_line(int wx, int wy, int64_t s, int64_t c, int dx, int dy, int64_t L2, int E, int K) {
    if (L2 == 0 || s <= 0) return draw_near(wx, wy, E);
    if (s >= L2) return draw_near(wx - dx, wy - dy, E);
    return (c < 0 ? -c : c) <= (int64_t)K;
}

__global__ __launch_bounds__(DRAW_THREADS) void k_draw_poses(DrawArgs a) {
    __shared__ int l_ax[DRAW_LIST], l_ay[DRAW_LIST], l_bx[DRAW_LIST], l_by[DRAW_LIST];
    __shared__ int l_reach[DRAW_LIST];                            // lines: K of draw_line_reach
    __shared__ unsigned l_kc[DRAW_LIST];
    __shared__ int l_wave[DRAW_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_x = (a.Wf + DRAW_TILE_W - 1) / DRAW_TILE_W;
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int tx0 = txi * DRAW_TILE_W, ty0 = tyi * DRAW_TILE_H;
    const int tx1 = tx0 + DRAW_TILE_W < a.Wf ? tx0 + DRAW_TILE_W : a.Wf, ty1 = ty0 + DRAW_TILE_H < a.Hf ? ty0 + DRAW_TILE_H : a.Hf;
    const int x0 = tx0 + (tid & 15) * DRAW_BLOCK_W, y0 = ty0 + (tid >> 4) * DRAW_BLOCK_H;
    const int wv = a.Wf - x0 < DRAW_BLOCK_W ? (a.Wf - x0 < 0 ? 0 : a.Wf - x0) : DRAW_BLOCK_W;        // the block's columns and rows inside the frame
    const int hv = a.Hf - y0 < DRAW_BLOCK_H ? (a.Hf - y0 < 0 ? 0 : a.Hf - y0) : DRAW_BLOCK_H;
    const bool whole = wv == DRAW_BLOCK_W && hv == DRAW_BLOCK_H, some = wv > 0 && hv > 0;
    const int N = a.R + 3 * a.S * a.P;                            // <= 8 + 96 P: P is held below 2^24 by the entry point
    const int E = (a.t * a.t) >> 2;
    for (int64_t f = blockIdx.y; f < a.n_frames; f += gridDim.y) {
        unsigned px[16];                                          // pixel (j, i) of the block at 8 j + i: channel 0 | channel 1 << 8 | channel 2 << 16
        unsigned done = 0;                                        // bit 8 j + i: painted, or outside the frame
        const unsigned char* src = a.frames + f * a.f_fs + (int64_t)y0 * a.f_rs + 3 * (int64_t)x0;
        if (a.vec_in && whole) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const DBytes24 v = *reinterpret_cast<const DBytes24*>(src + j * a.f_rs);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int b = 3 * i, w = b >> 2, sh = 8 * (b & 3);
                    unsigned q = v.e[w] >> sh;
                    if (sh > 8) q |= v.e[w + 1] << (32 - sh);
                    px[8 * j + i] = q & 0xFFFFFFu;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    px[8 * j + i] = 0u;
                    if (j < hv && i < wv) {
                        const unsigned char* q = src + j * a.f_rs + 3 * i;
                        px[8 * j + i] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
                    } else {
                        done |= 1u << (8 * j + i);
                    }
                }
        }
        const unsigned outside = done;
        // ---- bin a chunk, paint from it, from the last primitives to the first ----
        for (int base = N; base > 0; base -= DRAW_LIST) {
            const int i = base - DRAW_LIST + tid;
            int ax = 0, ay = 0, bx = 0, by = 0;
            int reach = 0;
            unsigned kc = 0u;
            const bool hit = i >= 0 && draw_decode(a, f, i, tx0, ty0, tx1, ty1, ax, ay, bx, by, kc, reach);
            const unsigned long long m = __ballot(hit);
            if (lane == 0) l_wave[wave] = __popcll(m);
            __syncthreads();
            int off = 0, n = 0;
#pragma unroll
            for (int w = 0; w < DRAW_THREADS / 64; ++w) {
                const int c = l_wave[w];
                off += w < wave ? c : 0;
                n += c;
            }
            if (hit) {
                const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
                l_ax[pos] = ax; l_ay[pos] = ay; l_bx[pos] = bx; l_by[pos] = by; l_kc[pos] = kc; l_reach[pos] = reach;
            }
            __syncthreads();                                      // (the next chunk's first barrier stands between these reads and its writes)
            for (int e = n - 1; e >= 0 && done != 0xFFFFu; --e) {
                const unsigned k = l_kc[e], kind = k >> 24, color = k & 0xFFFFFFu;
                const int Ax = l_ax[e], Ay = l_ay[e], Bx = l_bx[e], By = l_by[e];
                if (kind == KIND_FILL) {
                    if (Ax >= x0 + DRAW_BLOCK_W || Bx <= x0 || Ay >= y0 + DRAW_BLOCK_H || By <= y0) continue;
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (!(done >> (8 * j + i) & 1u) && x0 + i >= Ax && x0 + i < Bx && y0 + j >= Ay && y0 + j < By) {
                                px[8 * j + i] = color;
                                done |= 1u << (8 * j + i);
                            }
                } else if (kind == KIND_DOT) {
                    const int r = a.r;
                    if (Ax < x0 - r || Ax > x0 + DRAW_BLOCK_W - 1 + r || Ay < y0 - r || Ay > y0 + DRAW_BLOCK_H - 1 + r) continue;
                    const int wx = x0 - Ax, wy = y0 - Ay;         // after the cull |w| <= 7 + 32: the squares are small
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (!(done >> (8 * j + i) & 1u) && (wx + i) * (wx + i) + (wy + j) * (wy + j) <= r * r) {
                                px[8 * j + i] = color;
                                done |= 1u << (8 * j + i);
                            }
                } else {
                    const int h = (a.t + 1) >> 1;
                    if ((Ax < Bx ? Ax : Bx) - h > x0 + DRAW_BLOCK_W - 1 || (Ax < Bx ? Bx : Ax) + h < x0 || (Ay < By ? Ay : By) - h > y0 + DRAW_BLOCK_H - 1 ||
                        (Ay < By ? By : Ay) + h < y0)
                        continue;
                    const int dx = Bx - Ax, dy = By - Ay, wx = x0 - Ax, wy = y0 - Ay;
                    const int64_t L2 = (int64_t)dx * dx + (int64_t)dy * dy;
                    const int64_t s0 = (int64_t)wx * dx + (int64_t)wy * dy, c0 = (int64_t)wx * dy - (int64_t)wy * dx;
                    const int K = l_reach[e];
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if (!(done >> (8 * j + i) & 1u) &&
                                draw_on_line(wx + i, wy + j, s0 + (int64_t)i * dx + (int64_t)j * dy, c0 + (int64_t)i * dy - (int64_t)j * dx, dx, dy, L2, E, K)) {
                                px[8 * j + i] = color;
                                done |= 1u << (8 * j + i);
                            }
                }
            }
        }
        if (!some) continue;
        // ---- the painted frame ----
        if (a.out && !(a.in_place && done == outside)) {
            unsigned char* dst = a.out + f * a.o_fs + (int64_t)y0 * a.o_rs + 3 * (int64_t)x0;
            if (a.vec_out && whole) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    DBytes24 v;
#pragma unroll
                    for (int w = 0; w < 6; ++w) v.e[w] = 0u;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int b = 3 * i, w = b >> 2, sh = 8 * (b & 3);
                        v.e[w] |= px[8 * j + i] << sh;
                        if (sh > 8) v.e[w + 1] |= px[8 * j + i] >> (32 - sh);
                    }
                    *reinterpret_cast<DBytes24*>(dst + j * a.o_rs) = v;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (j < hv && i < wv) {
                            unsigned char* q = dst + j * a.o_rs + 3 * i;
                            q[0] = (unsigned char)(px[8 * j + i] & 255u);
                            q[1] = (unsigned char)((px[8 * j + i] >> 8) & 255u);
                            q[2] = (unsigned char)(px[8 * j + i] >> 16);
                        }
            }
        }
        if (!a.oy) continue;
        // ---- the surface, from the painted pixels (rule 5): at an odd edge the last column / row stands in for the missing one ----
        if (!whole) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 1; i < 8; i += 2)
                    if (i == wv) px[8 * j + i] = px[8 * j + i - 1];
            if (hv == 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) px[8 + i] = px[i];
            }
        }
        int sum[4][3];
        unsigned Y[2][2] = {{0u, 0u}, {0u, 0u}};
#pragma unroll
        for (int q = 0; q < 4; ++q) sum[q][0] = sum[q][1] = sum[q][2] = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c0 = (int)(px[8 * j + i] & 255u), c1 = (int)((px[8 * j + i] >> 8) & 255u), c2 = (int)(px[8 * j + i] >> 16);
                sum[i >> 1][0] += c0; sum[i >> 1][1] += c1; sum[i >> 1][2] += c2;
                const int y = dsat8((a.ky[0] * c0 + a.ky[1] * c1 + a.ky[2] * c2 + (a.yoff << 20) + (1 << 19)) >> 20);
                Y[j][i >> 2] |= (unsigned)y << (8 * (i & 3));
            }
        unsigned UV[2] = {0u, 0u};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int u = dsat8((a.ku[0] * sum[q][0] + a.ku[1] * sum[q][1] + a.ku[2] * sum[q][2] + (128 << 22) + (1 << 21)) >> 22);
            const int v = dsat8((a.kv[0] * sum[q][0] + a.kv[1] * sum[q][1] + a.kv[2] * sum[q][2] + (128 << 22) + (1 << 21)) >> 22);
            UV[q >> 1] |= ((unsigned)u | ((unsigned)v << 8)) << (16 * (q & 1));
        }
        unsigned char* dy = a.oy + f * a.y_fs + (int64_t)y0 * a.y_rs + x0;
        unsigned char* duv = a.ouv + f * a.uv_fs + (int64_t)(y0 >> 1) * a.uv_rs + x0;
        if (a.vec_y && whole) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                DBytes8 v;
                v.e[0] = Y[j][0]; v.e[1] = Y[j][1];
                *reinterpret_cast<DBytes8*>(dy + j * a.y_rs) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (j < hv && i < wv) dy[j * a.y_rs + i] = (unsigned char)((Y[j][i >> 2] >> (8 * (i & 3))) & 255u);
        }
        if (a.vec_uv && whole) {
            DBytes8 v;
            v.e[0] = UV[0]; v.e[1] = UV[1];
            *reinterpret_cast<DBytes8*>(duv) = v;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (2 * q < wv) {                                 // the pair is written whole: Wf rounded up to even
                    duv[2 * q] = (unsigned char)((UV[q >> 1] >> (16 * (q & 1))) & 255u);
                    duv[2 * q + 1] = (unsigned char)((UV[q >> 1] >> (16 * (q & 1) + 8)) & 255u);
                }
        }
    }
}

// kasf_pose_panel: one thread per joint; the stated order of single fp32 operations (no contraction: the intrinsics round each one)
__global__ __launch_bounds__(256) void k_pose_panel(const float* __restrict__ poses, int64_t n_joints, float ax0, float ax1, float ax2, float ay0, float ay1, float ay2,
                                                    float cx, float cy, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_joints; i += (int64_t)gridDim.x * 256) {
        const float* v = poses + 3 * i;
        const float* root = poses + 3 * (i / 17 * 17);
        const float dx = __fsub_rn(v[0], root[0]), dy = __fsub_rn(v[1], root[1]), dz = __fsub_rn(v[2], root[2]);
        out[2 * i] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(ax0, dx), __fmul_rn(ax1, dy)), __fmul_rn(ax2, dz)), cx);
        out[2 * i + 1] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(ay0, dx), __fmul_rn(ay1, dy)), __fmul_rn(ay2, dz)), cy);
    }
}

inline bool draw_on_grid(const void* p, int64_t a, int64_t b, int n) { return (((uintptr_t)p | (uintptr_t)a | (uintptr_t)b) & (uintptr_t)(n - 1)) == 0; }

}  // namespace

void kasf_launch_draw_poses(hipStream_t s, const KasfDrawLaunch* d) {
    if (d->n_frames <= 0) return;
    DrawArgs a;
    a.frames = (const unsigned char*)d->frames; a.f_rs = d->row_stride; a.f_fs = d->n_frames > 1 ? d->frame_stride : 0;
    a.out = (unsigned char*)d->out_bgr; a.o_rs = d->out_row_stride; a.o_fs = d->n_frames > 1 ? d->out_frame_stride : 0;
    a.oy = (unsigned char*)d->out_y; a.ouv = (unsigned char*)d->out_uv;
    a.y_rs = d->y_row_stride; a.uv_rs = d->uv_row_stride;
    a.y_fs = d->n_frames > 1 ? d->y_frame_stride : 0; a.uv_fs = d->n_frames > 1 ? d->uv_frame_stride : 0;
    a.kp = d->keypoints; a.kp_f = d->kp_frame_stride; a.kp_p = d->kp_person_stride; a.kp_j = d->kp_joint_stride; a.kp_c = d->kp_coord_stride;
    a.valid = d->valid; a.v_f = d->valid_frame_stride; a.v_p = d->valid_person_stride;
    a.seg = d->segments; a.col = d->colors; a.fills = d->fills;
    a.n_frames = d->n_frames; a.Hf = d->Hf; a.Wf = d->Wf; a.P = d->P; a.J = d->J; a.S = d->P > 0 ? d->S : 0; a.R = d->R;
    if (a.S == 0) a.P = 0;
    a.t = d->thickness; a.r = d->dot_radius; a.use_score = d->use_score; a.min_score = d->min_score;
    a.dot = (unsigned)d->dot_color[0] | ((unsigned)d->dot_color[1] << 8) | ((unsigned)d->dot_color[2] << 16);
    // coef = { CRY, CGY, CBY, CRU, CGU, CH, CGV, CBV } with CBU = CRV = CH (kasf.h, rule 5), placed by the frame's channel position
    const int* k = d->coef;
    const int r = d->rgb ? 0 : 2, b = 2 - r;
    a.ky[r] = k[0]; a.ky[1] = k[1]; a.ky[b] = k[2];
    a.ku[r] = k[3]; a.ku[1] = k[4]; a.ku[b] = k[5];
    a.kv[r] = k[5]; a.kv[1] = k[6]; a.kv[b] = k[7];
    a.yoff = d->full_range ? 0 : 16;
    a.vec_in = draw_on_grid(a.frames, a.f_rs, a.f_fs, 4);
    a.vec_out = a.out && draw_on_grid(a.out, a.o_rs, a.o_fs, 4);
    a.vec_y = a.oy && draw_on_grid(a.oy, a.y_rs, a.y_fs, 8);
    a.vec_uv = a.oy && draw_on_grid(a.ouv, a.uv_rs, a.uv_fs, 8);
    a.in_place = a.out == a.frames && a.o_rs == a.f_rs && a.o_fs == a.f_fs;
    const unsigned tiles = (unsigned)((d->Wf + DRAW_TILE_W - 1) / DRAW_TILE_W) * (unsigned)((d->Hf + DRAW_TILE_H - 1) / DRAW_TILE_H);      // <= 256 * 1024
    const dim3 grid(tiles, (unsigned)(d->n_frames > 65535 ? 65535 : d->n_frames)), block(DRAW_THREADS);
    hipLaunchKernelGGL(k_draw_poses, grid, block, 0, s, a);
}

void kasf_launch_pose_panel(hipStream_t s, const float* poses, int64_t n, const float view[8], float* out) {
    if (n <= 0) return;
    const int64_t joints = 17 * n, blocks = (joints + 255) / 256;
    const dim3 grid((unsigned)(blocks > 4096 ? 4096 : blocks)), block(256);
    hipLaunchKernelGGL(k_pose_panel, grid, block, 0, s, poses, joints, view[0], view[1], view[2], view[3], view[4], view[5], view[6], view[7], out);
}
