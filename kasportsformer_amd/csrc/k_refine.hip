// Recorded tracks refined with the frames after a gap known (kasf.h, kasf_tracks_refine): gaps of unusable joints filled by interpolation or a hold, then a
// symmetric, zero-phase weighted mean over the known joints of a window that never leaves the track.  The rule's three device functions are track_refine.h's.
//
// One launch.  A workgroup of four wavefronts owns kRefineTile consecutive PACKED frames and a chunk of JC joints; every frame finds its own track by a binary
// search of offsets, so a tile may span any number of short tracks.  With H = kRefineTile + 2 * radius:
//   0  per frame of [tile - radius, tile + kRefineTile + radius): its track [lo, hi), or none                         -> s_lo, s_hi [H]
//      the rows of those frames as they lie in memory, one float per lane: whole-row coalesced loads                  -> s_y [H][JC][Ct]
//   A  per (frame, joint): usable, or the fill; only a joint that is not usable walks up to max_gap frames each way, in global memory (L2)
//                                                                                                                     -> s_y in place, s_st [H][JC] bytes
//   B  per (tile frame, joint): the window out of LDS                                                                 -> s_o [kRefineTile][JC][Ct]
//   C  the tile's rows and states stored as they lie in memory: whole-row coalesced stores
// A frame's fill uses its own track's bounds and the window is clipped to min(radius, n - lo, hi - 1 - n), so everything phase B reads is inside the halo and
// inside the frame's track.  No atomics, no intermediate in global memory, every output element is written by one thread: the same bits from run to run, and a
// track's result does not depend on the other tracks of the launch.  The only device values that form an index are the offsets, clamped by refine_track_of.
// LDS: 16 H + 4 Ct JC (H + kRefineTile) + H JC + 144 bytes, JC chosen so that this stays within kRefineLds ("recorded-track refinement").
#include "kernels.h"

#ifndef KASF_DYNAMIC_LDS
#define KASF_DYNAMIC_LDS(name) extern __shared__ __attribute__((aligned(16))) float name[]
#endif

namespace {

constexpr int kRefineTile = 64, kRefineThreads = 256, kRefineLds = 48 * 1024;
constexpr int kRefineWPad = 36;                                    // the weights' 33 floats, padded to 16 bytes

__host__ __device__ inline int64_t refine_lds_fixed(int H) { return 16 * (int64_t)H + 4 * kRefineWPad; }
__host__ __device__ inline int64_t refine_lds_per_joint(int H, int Ct) { return 4 * (int64_t)Ct * (H + kRefineTile) + H; }

template <int C>
__global__ __launch_bounds__(kRefineThreads) void k_tracks_refine(const float* __restrict__ x, const int64_t* __restrict__ offsets, int64_t N, int P, int J,
                                                                  int has_score, KasfRefine p, int JC, float* __restrict__ out,
                                                                  unsigned char* __restrict__ state) {
    KASF_DYNAMIC_LDS(sm);
    const int Ct = C + (has_score ? 1 : 0), R = p.radius, H = kRefineTile + 2 * R, tid = threadIdx.x;
    const int row = JC * Ct;                                       // floats of a frame in s_y and s_o, whatever the chunk holds
    int64_t* s_lo = reinterpret_cast<int64_t*>(sm);
    int64_t* s_hi = s_lo + H;
    float* s_w = reinterpret_cast<float*>(s_hi + H);
    float* s_y = s_w + kRefineWPad;
    float* s_o = s_y + H * row;
    unsigned char* s_st = reinterpret_cast<unsigned char*>(s_o + kRefineTile * row);

    const int j0 = blockIdx.y * JC, jc = J - j0 < JC ? J - j0 : JC;                // this chunk's joints [j0, j0 + jc)
    const int64_t tiles = (N + kRefineTile - 1) / kRefineTile, stride = (int64_t)J * Ct;
    if (tid <= kRefineMaxRadius) s_w[tid] = p.w[tid];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t n0 = tile * kRefineTile, base = n0 - R;
        for (int h = tid; h < H; h += kRefineThreads) {
            const int64_t n = base + h;
            int64_t lo = -1, hi = -1;
            if (n < 0 || n >= N || !refine_track_of(offsets, P, N, n, lo, hi)) lo = hi = -1;
            s_lo[h] = lo;
            s_hi[h] = hi;
        }
        for (int e = tid; e < H * jc * Ct; e += kRefineThreads) {
            const int h = e / (jc * Ct), q = e - h * (jc * Ct);
            const int64_t n = base + h;
            s_y[h * row + q] = n >= 0 && n < N ? x[(n * J + j0) * Ct + q] : 0.0f;
        }
        __syncthreads();
        for (int e = tid; e < H * jc; e += kRefineThreads) {                       // phase A
            const int h = e / jc, jj = e - h * jc;
            const int64_t lo = s_lo[h], hi = s_hi[h];
            int st = kRefineLeft;
            if (lo >= 0) {
                float own[C + 1], y[C];
                float* yj = s_y + h * row + jj * Ct;
#pragma unroll
                for (int c = 0; c < C; ++c) own[c] = yj[c];
                own[C] = has_score ? yj[C] : 0.0f;
                st = refine_fill<C>(x + (int64_t)(j0 + jj) * Ct, stride, has_score != 0, p.min_score, p.max_gap, base + h, lo, hi, own, y);
                if (st == kRefineInterpolated || st == kRefineHeld) {
#pragma unroll
                    for (int c = 0; c < C; ++c) yj[c] = y[c];
                }
            }
            s_st[h * JC + jj] = (unsigned char)st;
        }
        __syncthreads();
        for (int e = tid; e < kRefineTile * jc; e += kRefineThreads) {             // phase B
            const int f = e / jc, jj = e - f * jc, h = f + R;
            const int64_t n = n0 + f, lo = s_lo[h], hi = s_hi[h];
            if (lo < 0) continue;                                                  // a row of no track, or past the end: not written
            const float* yj = s_y + h * row + jj * Ct;
            float* oj = s_o + f * row + jj * Ct;
            float o[C];
            if (s_st[h * JC + jj] < kRefineLeft) {
                int r = R;
                if (n - lo < r) r = (int)(n - lo);
                if (hi - 1 - n < r) r = (int)(hi - 1 - n);
                refine_smooth<C>(s_w, r, yj, row, s_st + h * JC + jj, JC, o);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) o[c] = yj[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) oj[c] = o[c];
            if (has_score) oj[C] = yj[C];
        }
        __syncthreads();
        for (int e = tid; e < kRefineTile * jc * Ct; e += kRefineThreads) {        // phase C
            const int f = e / (jc * Ct), q = e - f * (jc * Ct);
            if (s_lo[f + R] >= 0) out[((n0 + f) * J + j0) * Ct + q] = s_o[f * row + q];
        }
        if (state != nullptr)
            for (int e = tid; e < kRefineTile * jc; e += kRefineThreads) {
                const int f = e / jc, jj = e - f * jc;
                if (s_lo[f + R] >= 0) state[(n0 + f) * J + j0 + jj] = s_st[(f + R) * JC + jj];
            }
        __syncthreads();                                                           // the next tile overwrites what phase C reads
    }
}

template <int C>
void launch_refine(hipStream_t s, const float* x, const int64_t* offsets, int64_t N, int P, int J, int has_score, const KasfRefine& p, float* out,
                   unsigned char* state) {
    const int Ct = C + (has_score ? 1 : 0), H = kRefineTile + 2 * p.radius;
    int64_t JC = (kRefineLds - refine_lds_fixed(H)) / refine_lds_per_joint(H, Ct);          // >= 11 at the widest row and radius
    if (JC > J) JC = J;
    const int64_t tiles = (N + kRefineTile - 1) / kRefineTile, lds = refine_lds_fixed(H) + JC * refine_lds_per_joint(H, Ct);
    hipLaunchKernelGGL(k_tracks_refine<C>, dim3((unsigned)(tiles > 65536 ? 65536 : tiles), (unsigned)((J + JC - 1) / JC)), dim3(kRefineThreads), (size_t)lds, s,
                       x, offsets, N, P, J, has_score, p, (int)JC, out, state);
}

}  // namespace

// C in [1, 4], J in [1, 256], the radius and the gap as the entry point checked them: one instance per C keeps a joint's channels in registers
void kasf_launch_tracks_refine(hipStream_t s, const float* x, const int64_t* offsets, int64_t N, int P, int J, int C, int has_score, const KasfRefine& p, float* out,
                               unsigned char* state) {
    if (P <= 0 || N <= 0) return;
    switch (C) {
        case 1: launch_refine<1>(s, x, offsets, N, P, J, has_score, p, out, state); break;
        case 2: launch_refine<2>(s, x, offsets, N, P, J, has_score, p, out, state); break;
        case 3: launch_refine<3>(s, x, offsets, N, P, J, has_score, p, out, state); break;
        default: launch_refine<4>(s, x, offsets, N, P, J, has_score, p, out, state); break;
    }
}
