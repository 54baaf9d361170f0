// The One-Euro filter over keypoints [J][C + score] and poses [J][C] with its state on the device (kasf.h, kasf_one_euro_*): a live row per tick, its slot named
// by the host (k_one_euro_push) or read from the tracker's TrackResult (k_one_euro_tracked, kasf_stream_track_front's row rule), and whole recorded tracks with
// the state in registers (k_one_euro_tracks).  The step is one_euro.h's in all three, so a recorded track equals push called frame by frame bit for bit.
//
// One wavefront per row or track; a lane owns joints j, j + 64, ... and all C channels of each, because the gate is per joint.  Valid rows of a launch have
// distinct slots, so every xhat / dxhat / last / owner entry is read and written by one workgroup only: no atomics, no hand-off between workgroups, the same
// bits from run to run, and a row's result does not depend on the other rows of the launch.  Every index formed from a device value (slot id, count_b, slot,
// offset) is clamped into the arrays the host sized.  x is only read; out does not overlap it.
#include "kernels.h"

namespace {

constexpr int kAhead = 8;      // frames of a recorded track whose values are in registers ahead of the step

// Joint j of a row at x / out with state slot g (g < 0: no state, a copy-through).  last_known: the joint's last tick as the caller read or overrode it.
template <int C>
__device__ inline void smooth_joint_global(const KasfOneEuro& p, int has_score, const float* __restrict__ xj, int64_t tick, float* xhat_j, float* dxhat_j,
                                           int64_t* last_j, bool restart, float* __restrict__ oj) {
    float xh[C], dxh[C], o[C];
    int64_t last = restart ? -1 : *last_j;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xh[c] = xhat_j[c];
        dxh[c] = dxhat_j[c];
    }
    const bool stored = one_euro_joint<C>(p, has_score != 0, xj, tick, xh, dxh, last, o);
#pragma unroll
    for (int c = 0; c < C; ++c) oj[c] = o[c];
    if (has_score) oj[C] = xj[C];
    if (stored) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xhat_j[c] = xh[c];
            dxhat_j[c] = dxh[c];
        }
        *last_j = tick;
    } else if (restart) {
        *last_j = -1;
    }
}

// x, out [K][J][Ct]; row i -> slot slots[i] (NULL: i); an id outside [0, S) copies the row through.
template <int C>
__global__ __launch_bounds__(64) void k_one_euro_push(const float* __restrict__ x, const int* __restrict__ slots, int K, int S, int J, int has_score, KasfOneEuro p,
                                                      int64_t tick, float* xhat, float* dxhat, int64_t* last, float* __restrict__ out) {
    const int Ct = C + (has_score ? 1 : 0);
    for (int64_t row = blockIdx.x; row < K; row += gridDim.x) {
        const int64_t g = slots ? (int64_t)slots[row] : row;
        const bool valid = g >= 0 && g < S;
        const float* xr = x + row * J * Ct;
        float* orow = out + row * J * Ct;
        if (!valid) {
            for (int e = threadIdx.x; e < J * Ct; e += 64) orow[e] = xr[e];
            continue;
        }
        for (int j = threadIdx.x; j < J; j += 64) {
            const int64_t gj = g * J + j;
            smooth_joint_global<C>(p, has_score, xr + j * Ct, tick, xhat + gj * C, dxhat + gj * C, last + gj, false, orow + j * Ct);
        }
    }
}

// x, out [B * R][J][Ct]; the row's slot from the TrackResult arrays by kasf_stream_track_front's rule (tracked_rows.h); row_slot may be NULL.
template <int C>
__global__ __launch_bounds__(64) void k_one_euro_tracked(const float* __restrict__ x, const int* __restrict__ ids, const int* __restrict__ slot,
                                                         const int* __restrict__ born, const int* __restrict__ count_b, int B, int S_t, int rows_mode, int R, int J,
                                                         int has_score, KasfOneEuro p, int64_t tick, float* xhat, float* dxhat, int64_t* last, int* owner,
                                                         float* __restrict__ out, int* __restrict__ row_slot) {
    const int Ct = C + (has_score ? 1 : 0);
    const int64_t n_rows = (int64_t)B * R;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int b = (int)(row / R), k = (int)(row - (int64_t)b * R);
        const TrackedRow tr = tracked_row(ids, slot, born, count_b, b, k, S_t, rows_mode, owner);      // k < R by construction
        const bool valid = tr.valid, restart = tr.restart;
        const int64_t g = tr.g;
        __syncthreads();                                           // every lane has the old owner before lane 0 stores the new one
        if (threadIdx.x == 0) {
            if (restart) owner[g] = tr.id;
            if (row_slot) row_slot[row] = valid ? (int)g : -1;
        }
        const float* xr = x + row * J * Ct;
        float* orow = out + row * J * Ct;
        if (!valid) {
            for (int e = threadIdx.x; e < J * Ct; e += 64) orow[e] = xr[e];
            continue;
        }
        for (int j = threadIdx.x; j < J; j += 64) {                // a joint's last entry is its lane's alone: a restart writes -1 where the step stores nothing
            const int64_t gj = g * J + j;
            smooth_joint_global<C>(p, has_score, xr + j * Ct, tick, xhat + gj * C, dxhat + gj * C, last + gj, restart, orow + j * Ct);
        }
    }
}

// x, out [N][J][Ct]; track t = frames [offsets[t], offsets[t + 1]) (clamped into [0, N] and to a non-negative length), every track from an empty state,
// tick = frame index within the track.  A joint's state lives in its lane's registers over the whole track.
template <int C>
__global__ __launch_bounds__(64) void k_one_euro_tracks(const float* __restrict__ x, const int64_t* __restrict__ offsets, int64_t N, int P, int J, int has_score,
                                                        KasfOneEuro p, float* __restrict__ out) {
    const int Ct = C + (has_score ? 1 : 0);
    for (int t = blockIdx.x; t < P; t += gridDim.x) {
        const int64_t f0 = lift_clamp(offsets[t], 0, N), f1 = lift_clamp(offsets[t + 1], f0, N);
        for (int j = threadIdx.x; j < J; j += 64) {
            float xh[C], dxh[C], o[C];
#pragma unroll
            for (int c = 0; c < C; ++c) xh[c] = dxh[c] = 0.0f;
            int64_t last = -1;
            // the step is a chain from frame to frame, the loads are not: kAhead frames' values are fetched before the chain walks them
            for (int64_t fb = f0; fb < f1; fb += kAhead) {
                float in[kAhead][C + 1];
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const float* xj = x + (lift_clamp(fb + u, f0, f1 - 1) * J + j) * Ct;
#pragma unroll
                    for (int c = 0; c < C; ++c) in[u][c] = xj[c];
                    in[u][C] = has_score ? xj[C] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < kAhead; ++u) {
                    const int64_t f = fb + u;
                    if (f >= f1) break;
                    float* oj = out + (f * J + j) * Ct;
                    one_euro_joint<C>(p, has_score != 0, in[u], f - f0, xh, dxh, last, o);
#pragma unroll
                    for (int c = 0; c < C; ++c) oj[c] = o[c];
                    if (has_score) oj[C] = in[u][C];
                }
            }
        }
    }
}

template <int C>
void launch_push(hipStream_t s, const float* x, const int* slots, int K, int S, int J, int has_score, const KasfOneEuro& p, int64_t tick, float* xhat, float* dxhat,
                 int64_t* last, float* out) {
    hipLaunchKernelGGL(k_one_euro_push<C>, dim3((unsigned)(K > 65536 ? 65536 : K)), dim3(64), 0, s, x, slots, K, S, J, has_score, p, tick, xhat, dxhat, last, out);
}

template <int C>
void launch_tracked(hipStream_t s, const float* x, const int* ids, const int* slot, const int* born, const int* count_b, int B, int S_t, int rows_mode, int R, int J,
                    int has_score, const KasfOneEuro& p, int64_t tick, float* xhat, float* dxhat, int64_t* last, int* owner, float* out, int* row_slot) {
    const int64_t n_rows = (int64_t)B * R;
    hipLaunchKernelGGL(k_one_euro_tracked<C>, dim3((unsigned)(n_rows > 65536 ? 65536 : n_rows)), dim3(64), 0, s, x, ids, slot, born, count_b, B, S_t, rows_mode, R,
                       J, has_score, p, tick, xhat, dxhat, last, owner, out, row_slot);
}

template <int C>
void launch_tracks(hipStream_t s, const float* x, const int64_t* offsets, int64_t N, int P, int J, int has_score, const KasfOneEuro& p, float* out) {
    hipLaunchKernelGGL(k_one_euro_tracks<C>, dim3((unsigned)(P > 65536 ? 65536 : P)), dim3(64), 0, s, x, offsets, N, P, J, has_score, p, out);
}

}  // namespace

// C in [1, 4] as the entry points checked it: one instance per C keeps a joint's channels in registers
#define KASF_ONE_EURO_BY_C(call)      \
    switch (C) {                      \
        case 1: call(1); break;       \
        case 2: call(2); break;       \
        case 3: call(3); break;       \
        default: call(4); break;      \
    }

void kasf_launch_one_euro_push(hipStream_t s, const float* x, const int* slots, int K, int S, int J, int C, int has_score, const KasfOneEuro& p, int64_t tick,
                               float* xhat, float* dxhat, int64_t* last, float* out) {
    if (K <= 0) return;
#define KASF_CALL(c) launch_push<c>(s, x, slots, K, S, J, has_score, p, tick, xhat, dxhat, last, out)
    KASF_ONE_EURO_BY_C(KASF_CALL)
#undef KASF_CALL
}

void kasf_launch_one_euro_tracked(hipStream_t s, const float* x, const int* ids, const int* slot, const int* born, const int* count_b, int B, int S_t, int rows_mode,
                                  int R, int J, int C, int has_score, const KasfOneEuro& p, int64_t tick, float* xhat, float* dxhat, int64_t* last, int* owner,
                                  float* out, int* row_slot) {
    if ((int64_t)B * R <= 0) return;
#define KASF_CALL(c) launch_tracked<c>(s, x, ids, slot, born, count_b, B, S_t, rows_mode, R, J, has_score, p, tick, xhat, dxhat, last, owner, out, row_slot)
    KASF_ONE_EURO_BY_C(KASF_CALL)
#undef KASF_CALL
}

void kasf_launch_one_euro_tracks(hipStream_t s, const float* x, const int64_t* offsets, int64_t N, int P, int J, int C, int has_score, const KasfOneEuro& p,
                                 float* out) {
    if (P <= 0) return;
#define KASF_CALL(c) launch_tracks<c>(s, x, offsets, N, P, J, has_score, p, out)
    KASF_ONE_EURO_BY_C(KASF_CALL)
#undef KASF_CALL
}
