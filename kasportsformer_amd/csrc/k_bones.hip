// Constant limb lengths per player (kasf.h, kasf_bone_*): the per-track lower median of every bone's length (k_bone_lengths, k_bone_select), the walk from the
// root that re-imposes a table of lengths on every frame (k_bone_apply), and the live form with a running mean per slot in device memory, its slot named by the
// host (k_bone_push) or read from the tracker's TrackResult (k_bone_tracked, by tracked_rows.h's rule).  bone_walk / bone_symmetric are the one
// definition of the walk; every fp32 line is the rounded operation(s) kasf.h names, left to right (-ffp-contract=off, correctly rounded divide and square root).
//
// The two frame kernels move 204 B per frame in (and out): a workgroup stages BONE_TILE frames in LDS as k_pose.hip does -- global loads and stores are one
// float4 per lane on consecutive addresses, lane i then owns frame i at LDS stride 51 (odd: no bank is shared) with its 17 joints in registers -- and the grid
// walks the packed array, so one track of 18,000 frames and 200 tracks of 40 are the same launch.  The lengths go to the caller's scratch bone-major
// ([16][N], an unusable one as 0) so that the select reads a (track, bone) as one contiguous run.
//
// The select is a radix select over the bit patterns (positive floats order as uint32): four passes of 8 bits, one workgroup of 256 per (track, bone), a
// 256-bin histogram in LDS filled with integer atomics, and after each pass every wave scans the bins alike (lane l holds bins 4 l .. 4 l + 3) and keeps the bin
// that holds the rank.  The median is an order statistic: its bits do not depend on the order the counts arrive in, so the result is the same from run to run.
// Every index formed from a device value (offset, slot id, count_b, slot) is clamped into the arrays the host sized.  Inputs are only read.
#include "kernels.h"
#include "bone_table.h"

namespace {

constexpr int BONE_TILE = 128;                                  // frames per workgroup pass = threads per workgroup; 128 * 204 B = 25.5 KiB of LDS
constexpr int BONE_TILE_FLOATS = BONE_TILE * 51;                // a multiple of 4: every full tile starts 16-byte aligned when the array does
constexpr int SELECT_THREADS = 256;                             // = the bins of a pass

__device__ inline bool bone_finite(float v) { return fabsf(v) <= 3.4028235e38f; }                // false for a NaN and for an infinity
__device__ inline bool bone_usable(float l) { return l > 0.0f && l <= 3.4028235e38f; }
__device__ inline float bone_len(float vx, float vy, float vz) { return sqrtf((vx * vx + vy * vy) + vz * vz); }
__device__ inline unsigned bone_bits(float v) { return __builtin_bit_cast(unsigned, v); }

// the table before use: a pair gets (La + Lb) * 0.5f, or the one that is set; an entry that is not > 0 counts as 0
__device__ inline float bone_pair(float La, float Lb) { return La > 0.0f && Lb > 0.0f ? (La + Lb) * 0.5f : (La > 0.0f ? La : (Lb > 0.0f ? Lb : 0.0f)); }
__device__ inline void bone_symmetric(float (&L)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (bone_partner(k) > k) L[k] = L[bone_partner(k)] = bone_pair(L[k], L[bone_partner(k)]);
}

// y[0] = x[0]; bone k ascending: y[child] = y[parent] + v * (L / l) where L > 0 and l is usable, else y[parent] + v
__device__ inline void bone_walk(const float (&x)[17][3], const float (&L)[16], float (&y)[17][3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) y[0][c] = x[0][c];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int ch = k + 1, pa = bone_parent(k);
        const float vx = x[ch][0] - x[pa][0], vy = x[ch][1] - x[pa][1], vz = x[ch][2] - x[pa][2];
        const float l = bone_len(vx, vy, vz);
        if (L[k] > 0.0f && bone_usable(l)) {
            const float s = L[k] / l;
            y[ch][0] = y[pa][0] + vx * s;
            y[ch][1] = y[pa][1] + vy * s;
            y[ch][2] = y[pa][2] + vz * s;
        } else {
            y[ch][0] = y[pa][0] + vx;
            y[ch][1] = y[pa][1] + vy;
            y[ch][2] = y[pa][2] + vz;
        }
    }
}

// frames [first, first + count) of src -> LDS tile (and back): VEC = the float4 form, for full tiles of 16-byte aligned arrays
template <bool VEC>
__device__ inline void tile_load(const float* __restrict__ src, int64_t first, int count, float* tile) {
    if (VEC && count == BONE_TILE) {
        const float4* s4 = reinterpret_cast<const float4*>(src + first * 51);
        float4* t4 = reinterpret_cast<float4*>(tile);
        for (int i = threadIdx.x; i < BONE_TILE_FLOATS / 4; i += BONE_TILE) t4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < count * 51; i += BONE_TILE) tile[i] = src[first * 51 + i];
    }
}
template <bool VEC>
__device__ inline void tile_store(const float* tile, int64_t first, int count, float* __restrict__ dst) {
    if (VEC && count == BONE_TILE) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* d4 = reinterpret_cast<float4*>(dst + first * 51);
        for (int i = threadIdx.x; i < BONE_TILE_FLOATS / 4; i += BONE_TILE) d4[i] = t4[i];
    } else {
        for (int i = threadIdx.x; i < count * 51; i += BONE_TILE) dst[first * 51 + i] = tile[i];
    }
}

// a frame of the tile into registers -> whether all its 51 values are finite
__device__ inline bool frame_load(const float* f, float (&x)[17][3]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 17; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[j][c] = f[3 * j + c];
            ok = ok && bone_finite(x[j][c]);
        }
    return ok;
}

// poses [N][17][3] -> scratch [16][N]: bone k's length in frame f, 0 where the frame or the length is not usable
template <bool VEC>
__global__ __launch_bounds__(BONE_TILE) void k_bone_lengths(const float* __restrict__ poses, int64_t N, float* __restrict__ scratch) {
    __shared__ __attribute__((aligned(16))) float tile[BONE_TILE_FLOATS];
    const int64_t tiles = (N + BONE_TILE - 1) / BONE_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * BONE_TILE;
        const int count = (int)(N - first < BONE_TILE ? N - first : BONE_TILE);
        tile_load<VEC>(poses, first, count, tile);
        __syncthreads();
        if ((int)threadIdx.x < count) {
            float x[17][3];
            const bool ok = frame_load(tile + threadIdx.x * 51, x);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int ch = k + 1, pa = bone_parent(k);
                const float l = bone_len(x[ch][0] - x[pa][0], x[ch][1] - x[pa][1], x[ch][2] - x[pa][2]);
                scratch[(int64_t)k * N + first + threadIdx.x] = ok && bone_usable(l) ? l : 0.0f;       // consecutive lanes, consecutive addresses
            }
        }
        __syncthreads();                                        // the next pass overwrites the tile
    }
}

// scratch [16][N], track p = frames [offsets[p], offsets[p + 1]) clamped as k_one_euro_tracks clamps them -> lengths [P][16] = the element of rank (n - 1) / 2
// among the n usable lengths (0 for n = 0), counts [P][16] = n (may be null).  One workgroup per (track, bone).
__global__ __launch_bounds__(SELECT_THREADS) void k_bone_select(const float* __restrict__ scratch, const int64_t* __restrict__ offsets, int64_t N, int P,
                                                                float* __restrict__ lengths, int* __restrict__ counts) {
    __shared__ int hist[SELECT_THREADS];
    const int lane = threadIdx.x & 63;
    for (int64_t item = blockIdx.x; item < (int64_t)P * 16; item += gridDim.x) {
        const int p = (int)(item >> 4), k = (int)(item & 15);
        const int64_t f0 = lift_clamp(offsets[p], 0, N), f1 = lift_clamp(offsets[p + 1], f0, N);
        const float* v = scratch + (int64_t)k * N;
        unsigned prefix = 0, mask = 0;                          // the median's bits found so far, and which bits those are
        int rank = 0, n = 0;                                    // the rank wanted among the values that match prefix under mask
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            hist[threadIdx.x] = 0;
            __syncthreads();
            for (int64_t f = f0 + threadIdx.x; f < f1; f += SELECT_THREADS) {
                const unsigned u = bone_bits(v[f]);
                if (u - 1u < 0x7F7FFFFFu && (u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);      // u in [1, 0x7F7FFFFF]: positive and finite
            }
            __syncthreads();
            // every wave scans the 256 bins alike, so the rank and the prefix stay in registers, uniform over the workgroup
            const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const int own = (h0 + h1) + (h2 + h3);
            int incl = own;
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl(incl, lane - d);
                if (lane >= d) incl += up;
            }
            if (pass == 0) {
                n = __shfl(incl, 63);
                rank = n > 0 ? (n - 1) / 2 : 0;
            }
            int src = __popcll(__ballot(incl <= rank));         // incl ascends: the first lane whose bins reach past the rank (n = 0: none does)
            src = src > 63 ? 63 : src;
            int b = 4 * lane, r = rank - (incl - own);
            if (r >= h0) {
                r -= h0, ++b;
                if (r >= h1) {
                    r -= h1, ++b;
                    if (r >= h2) r -= h2, ++b;
                }
            }
            b = __shfl(b, src);
            rank = __shfl(r, src);
            prefix |= (unsigned)b << shift;
            mask |= 255u << shift;
            __syncthreads();                                    // every wave has read the bins before the next pass clears them
        }
        if (threadIdx.x == 0) {
            lengths[item] = n > 0 ? __builtin_bit_cast(float, prefix) : 0.0f;
            if (counts) counts[item] = n;
        }
    }
}

// poses, out [N][17][3]; lengths [P][16] with offsets [P + 1] (per_track) or one [16] for every frame.  A frame of no track, or one that is not usable, is
// copied through bit for bit.
template <bool VEC>
__global__ __launch_bounds__(BONE_TILE) void k_bone_apply(const float* __restrict__ poses, const int64_t* __restrict__ offsets, int64_t N, int P,
                                                          const float* __restrict__ lengths, int per_track, int symmetric, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[BONE_TILE_FLOATS];
    const int64_t tiles = (N + BONE_TILE - 1) / BONE_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * BONE_TILE;
        const int count = (int)(N - first < BONE_TILE ? N - first : BONE_TILE);
        tile_load<VEC>(poses, first, count, tile);
        __syncthreads();
        if ((int)threadIdx.x < count) {
            const int64_t f = first + threadIdx.x;
            int p = 0;
            bool mine = true;
            if (per_track) {                                    // p = how many of offsets[1 .. P] are <= f (they ascend): always an index into the table
                int lo = 0, hi = P;
                while (lo < hi) {
                    const int mid = lo + (hi - lo + 1) / 2;
                    if (offsets[mid] <= f) lo = mid;
                    else hi = mid - 1;
                }
                mine = lo < P && offsets[lo] <= f;
                p = lo < P ? lo : P - 1;
            }
            float* fr = tile + threadIdx.x * 51;
            float x[17][3], y[17][3], L[16];
            if (frame_load(fr, x) && mine) {
#pragma unroll
                for (int k = 0; k < 16; ++k) L[k] = lengths[(int64_t)p * 16 + k];
                if (symmetric) bone_symmetric(L);
                bone_walk(x, L, y);
#pragma unroll
                for (int j = 0; j < 17; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) fr[3 * j + c] = y[j][c];
            }
        }
        __syncthreads();
        tile_store<VEC>(tile, first, count, out);
        __syncthreads();                                        // the next pass overwrites the tile
    }
}

// ---- the live form: one wavefront per row; state len [S][16] fp32, cnt [S][16] int32 ----
struct BoneLds {
    float x[51], tab[16], scale[16];
};

// One row with state slot g (g < 0: a copy-through), all 64 lanes.  Valid rows of a launch have distinct g, so this workgroup alone touches the slot.
// restart: the slot starts again (cnt = 0) whatever the frame holds.  Lane k < 16 owns bone k's length and state, lane c < 3 walks channel c.
__device__ inline void bone_live_row(BoneLds& s, const float* __restrict__ xr, float* __restrict__ orow, int64_t g, bool restart, int window, int symmetric,
                                     float* len, int* cnt) {
    const int lane = threadIdx.x;
    const float xv = lane < 51 ? xr[lane] : 0.0f;
    __syncthreads();                                            // the row before this one has been walked
    if (lane < 51) s.x[lane] = xv;
    const bool unusable = __syncthreads_or(lane < 51 && !bone_finite(xv) ? 1 : 0) != 0;
    if (g < 0 || unusable) {                                    // uniform over the workgroup
        if (lane < 51) orow[lane] = xv;
        if (g >= 0 && restart && lane < 16) cnt[g * 16 + lane] = 0;
        return;
    }
    float l = 0.0f;
    if (lane < 16) {
        const int ch = lane + 1, pa = bone_parent(lane);
        l = bone_len(s.x[3 * ch] - s.x[3 * pa], s.x[3 * ch + 1] - s.x[3 * pa + 1], s.x[3 * ch + 2] - s.x[3 * pa + 2]);
        int n = restart ? 0 : cnt[g * 16 + lane];
        float m = len[g * 16 + lane];                           // means something only where n > 0
        if (bone_usable(l)) {
            const int d = n + 1 < window ? n + 1 : window;
            m = n == 0 ? l : m + (l - m) / (float)d;
            n = d;
            len[g * 16 + lane] = m;
            cnt[g * 16 + lane] = n;
        } else if (restart) {
            cnt[g * 16 + lane] = 0;
        }
        s.tab[lane] = n > 0 ? m : 0.0f;
    }
    __syncthreads();
    if (lane < 16) {
        float L = s.tab[lane];
        if (symmetric && bone_partner(lane) != lane) L = bone_pair(L, s.tab[bone_partner(lane)]);      // a + b = b + a: both partners get the same bits
        s.scale[lane] = L > 0.0f && bone_usable(l) ? L / l : -1.0f;                                    // a scale is never negative: -1 = leave the bone as it is
    }
    __syncthreads();
    if (lane < 3) {
        float y[17];
        y[0] = s.x[lane];
        orow[lane] = y[0];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int ch = k + 1, pa = bone_parent(k);
            const float v = s.x[3 * ch + lane] - s.x[3 * pa + lane], sc = s.scale[k];
            y[ch] = sc >= 0.0f ? y[pa] + v * sc : y[pa] + v;
            orow[3 * ch + lane] = y[ch];
        }
    }
}

// x, out [K][17][3]; row i -> slot slots[i] (NULL: i); an id outside [0, S) copies the row through
__global__ __launch_bounds__(64) void k_bone_push(const float* __restrict__ x, const int* __restrict__ slots, int K, int S, int window, int symmetric, float* len,
                                                  int* cnt, float* __restrict__ out) {
    __shared__ BoneLds s;
    for (int64_t row = blockIdx.x; row < K; row += gridDim.x) {
        const int64_t g = slots ? (int64_t)slots[row] : row;
        bone_live_row(s, x + row * 51, out + row * 51, g >= 0 && g < S ? g : -1, false, window, symmetric, len, cnt);
    }
}

// x, out [B * R][17][3]; the row's slot from the TrackResult arrays by kasf_stream_track_front's rule (tracked_rows.h).  row_slot may be NULL.
__global__ __launch_bounds__(64) void k_bone_tracked(const float* __restrict__ x, const int* __restrict__ ids, const int* __restrict__ slot,
                                                     const int* __restrict__ born, const int* __restrict__ count_b, int B, int S_t, int rows_mode, int R, int window,
                                                     int symmetric, float* len, int* cnt, int* owner, float* __restrict__ out, int* __restrict__ row_slot) {
    __shared__ BoneLds sh;
    const int64_t n_rows = (int64_t)B * R;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int b = (int)(row / R), k = (int)(row - (int64_t)b * R);
        const TrackedRow tr = tracked_row(ids, slot, born, count_b, b, k, S_t, rows_mode, owner);      // k < R by construction
        __syncthreads();                                           // every lane has the old owner before lane 0 stores the new one
        if (threadIdx.x == 0) {
            if (tr.restart) owner[tr.g] = tr.id;
            if (row_slot) row_slot[row] = tr.valid ? (int)tr.g : -1;
        }
        bone_live_row(sh, x + row * 51, out + row * 51, tr.valid ? tr.g : -1, tr.restart, window, symmetric, len, cnt);
    }
}

inline unsigned tiles_grid(int64_t frames) {
    const int64_t g = (frames + BONE_TILE - 1) / BONE_TILE;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
inline bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace

void kasf_launch_bone_lengths(hipStream_t s, const float* poses, int64_t N, float* scratch) {
    if (N <= 0) return;
    if (aligned16(poses, poses)) hipLaunchKernelGGL(k_bone_lengths<true>, dim3(tiles_grid(N)), dim3(BONE_TILE), 0, s, poses, N, scratch);
    else hipLaunchKernelGGL(k_bone_lengths<false>, dim3(tiles_grid(N)), dim3(BONE_TILE), 0, s, poses, N, scratch);
}

void kasf_launch_bone_select(hipStream_t s, const float* scratch, const int64_t* offsets, int64_t N, int P, float* lengths, int* counts) {
    if (P <= 0) return;
    const int64_t items = (int64_t)P * 16;
    hipLaunchKernelGGL(k_bone_select, dim3((unsigned)(items > 65536 ? 65536 : items)), dim3(SELECT_THREADS), 0, s, scratch, offsets, N, P, lengths, counts);
}

void kasf_launch_bone_apply(hipStream_t s, const float* poses, const int64_t* offsets, int64_t N, int P, const float* lengths, int per_track, int symmetric,
                            float* out) {
    if (N <= 0) return;
    if (aligned16(poses, out))
        hipLaunchKernelGGL(k_bone_apply<true>, dim3(tiles_grid(N)), dim3(BONE_TILE), 0, s, poses, offsets, N, P, lengths, per_track, symmetric, out);
    else
        hipLaunchKernelGGL(k_bone_apply<false>, dim3(tiles_grid(N)), dim3(BONE_TILE), 0, s, poses, offsets, N, P, lengths, per_track, symmetric, out);
}

void kasf_launch_bone_push(hipStream_t s, const float* x, const int* slots, int K, int S, int window, int symmetric, float* len, int* cnt, float* out) {
    if (K <= 0) return;
    hipLaunchKernelGGL(k_bone_push, dim3((unsigned)(K > 65536 ? 65536 : K)), dim3(64), 0, s, x, slots, K, S, window, symmetric, len, cnt, out);
}

void kasf_launch_bone_tracked(hipStream_t s, const float* x, const int* ids, const int* slot, const int* born, const int* count_b, int B, int S_t, int rows_mode,
                              int R, int window, int symmetric, float* len, int* cnt, int* owner, float* out, int* row_slot) {
    const int64_t n_rows = (int64_t)B * R;
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(k_bone_tracked, dim3((unsigned)(n_rows > 65536 ? 65536 : n_rows)), dim3(64), 0, s, x, ids, slot, born, count_b, B, S_t, rows_mode, R, window,
                       symmetric, len, cnt, owner, out, row_slot);
}
