// The rule of kasf_tracks_refine (kasf.h): which track a packed frame belongs to, the gap fill of one joint and the symmetric smoothing of one joint, as
// k_refine.hip's kernel uses them.  "Usable" is one_euro.h's test, the same code.  The library is built with -ffp-contract=off and a correctly rounded divide:
// every line below is the rounded fp32 operation(s) kasf.h names, left to right.  Nothing here calls a transcendental: the weights are the host's.
// Plain C++: HIP device code in the library, g++ behind the stand-in hip/hip_runtime.h of tests/host_emul/ in the CPU tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lift_math.h"   // lift_clamp
#include "one_euro.h"    // joint_usable

constexpr int kRefineMaxGap = 64, kRefineMaxRadius = 32;

// kasf_refine_params of kasf.h as the kernel receives it: by value in the launch arguments
struct KasfRefine {
    float min_score;
    int max_gap, radius;
    float w[kRefineMaxRadius + 1];
};

// refine_fill's result, the values of the state output
enum : int { kRefineUsable = 0, kRefineInterpolated = 1, kRefineHeld = 2, kRefineLeft = 3 };

// The track of packed frame n, 0 <= n < N: the last p whose clamped start is <= n, if n is before its clamped end -> [lo, hi) with lo <= n < hi.  offsets [P + 1]
// ascend; whatever they hold, only offsets[0 .. P] are read and 0 <= lo <= n < hi <= N holds when the answer is true.
__device__ inline bool refine_track_of(const int64_t* __restrict__ offsets, int P, int64_t N, int64_t n, int64_t& lo, int64_t& hi) {
    int a = 0, b = P;                                              // the starts of tracks [0, a) are <= n, those of [b, P) are not
    while (a < b) {
        const int m = a + (b - a) / 2;
        if (lift_clamp(offsets[m], 0, N) <= n) a = m + 1;
        else b = m;
    }
    if (a == 0) return false;
    lo = lift_clamp(offsets[a - 1], 0, N);
    hi = lift_clamp(offsets[a], lo, N);
    return lo <= n && n < hi;
}

// Step 2 for one joint of frame n of track [lo, hi).  xj: the joint's column of the packed input, frame m's values at xj + m * stride; own: the Ct values of
// frame n.  Writes the filled y (the input as it came for state 0 and 3) and returns the state.  A search stops after max_gap frames or at the track's end,
// whichever is nearer: a neighbour farther away makes the gap longer than max_gap whatever the other side holds.
template <int C>
__device__ inline int refine_fill(const float* __restrict__ xj, int64_t stride, bool has_score, float min_score, int max_gap, int64_t n, int64_t lo, int64_t hi,
                                  const float* own, float (&y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = own[c];
    if (joint_usable<C>(own, has_score, min_score)) return kRefineUsable;
    const int64_t first = n - lo <= max_gap ? lo : n - max_gap, last = hi - 1 - n <= max_gap ? hi - 1 : n + max_gap;
    int64_t a = -1, b = -1;
    for (int64_t m = n - 1; m >= first; --m)
        if (joint_usable<C>(xj + m * stride, has_score, min_score)) {
            a = m;
            break;
        }
    for (int64_t m = n + 1; m <= last; ++m)
        if (joint_usable<C>(xj + m * stride, has_score, min_score)) {
            b = m;
            break;
        }
    if (a >= 0 && b >= 0) {
        if (b - a - 1 > max_gap) return kRefineLeft;
        const float t = (float)(n - a) / (float)(b - a);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float xa = xj[a * stride + c], xb = xj[b * stride + c];
            y[c] = xa + (xb - xa) * t;
        }
        return kRefineInterpolated;
    }
    int64_t from = -1;
    if (a < 0 && b >= 0 && first == lo && b - lo <= max_gap) from = b;             // a leading run: [lo, n) was searched whole
    if (b < 0 && a >= 0 && last == hi - 1 && hi - 1 - a <= max_gap) from = a;       // a trailing run: (n, hi) was searched whole
    if (from < 0) return kRefineLeft;
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = xj[from * stride + c];
    return kRefineHeld;
}

// Step 3 for one known joint.  yn: its filled values at frame n, frame n + k's at yn + k * ystride; sn: its state at frame n, frame n + k's at sn[k * sstride];
// r: the window's half width, already min(radius, n - lo, hi - 1 - n); w: the weights by distance.
template <int C>
__device__ inline void refine_smooth(const float* w, int r, const float* yn, int ystride, const unsigned char* sn, int sstride, float (&out)[C]) {
    float y0[C], num[C], den = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        y0[c] = yn[c];
        num[c] = 0.0f;
    }
    for (int k = -r; k <= r; ++k) {
        if (sn[k * sstride] >= kRefineLeft) continue;
        const float wk = w[k < 0 ? -k : k];
#pragma unroll
        for (int c = 0; c < C; ++c) num[c] = num[c] + wk * (yn[k * ystride + c] - y0[c]);
        den = den + wk;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = y0[c] + num[c] / den;
}
