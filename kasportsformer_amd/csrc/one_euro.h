// The One-Euro step (Casiez, Roussel, Vogel, CHI 2012) that the three kernels of k_smooth.hip share (kasf.h, kasf_one_euro_*; the row rule of the
// tracker-driven entry is tracked_rows.h's): one definition of "usable", of the tick distance, of the hold and of the update, so that "a recorded track equals push called
// frame by frame" holds bit for bit.  The library is built with -ffp-contract=off and a correctly rounded divide: every line below is the rounded fp32
// operation(s) kasf.h names, left to right.
// Plain C++: HIP device code in the library, g++ behind the stand-in hip/hip_runtime.h of tests/host_emul/ in the CPU tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// kasf_one_euro_params of kasf.h as the kernels receive it: by value in the launch arguments
struct KasfOneEuro {
    float dt, min_cutoff, d_cutoff, beta, min_score;
    int max_hold;
};

// Whether a joint can be used: x: its Ct = C + has_score values.  Every one of the C values finite and within 1e12, and (with a score) the score at least
// min_score.  The one statement of the test for the One-Euro step and for the recorded-track refinement (track_refine.h).
template <int C>
__device__ inline bool joint_usable(const float* x, bool has_score, float min_score) {
    bool usable = true;
#pragma unroll
    for (int c = 0; c < C; ++c) usable = usable && fabsf(x[c]) <= 1e12f;       // false for a NaN and for an infinity as well: finite and within 1e12
    if (has_score) usable = usable && x[C] >= min_score;           // a NaN score fails the comparison
    return usable;
}

// One joint of one row.  x: the joint's Ct = C + has_score input values; xh, dxh: its estimate and derivative (read only when last >= 0); last: the tick of its
// last update, < 0 for none.  Writes the C filtered channels to out (the score channel is the caller's copy) and returns whether xh / dxh / last changed: they
// are to be stored exactly then, a held joint's state stays as it is.
template <int C>
__device__ inline bool one_euro_joint(const KasfOneEuro& p, bool has_score, const float* x, int64_t tick, float (&xh)[C], float (&dxh)[C], int64_t& last,
                                      float (&out)[C]) {
    float m[C];
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = x[c];
    const bool usable = joint_usable<C>(x, has_score, p.min_score);
    int64_t k = tick - last;
    if (k < 1) k = 1;
    const bool have = last >= 0 && k - 1 <= (int64_t)p.max_hold;   // an estimate older than max_hold missed ticks is dropped
    if (!have) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = m[c];
        if (!usable) return false;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            xh[c] = m[c];
            dxh[c] = 0.0f;
        }
        last = tick;
        return true;
    }
    if (!usable) {                                                 // hold
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = xh[c];
        return false;
    }
    const float two_pi = 6.2831855f;
    const float dtj = (float)k * p.dt;
    const float rd = two_pi * p.d_cutoff * dtj;
    const float ad = rd / (rd + 1.0f);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float d = (m[c] - xh[c]) / dtj;
        const float dx = dxh[c] + ad * (d - dxh[c]);
        const float fc = p.min_cutoff + p.beta * fabsf(dx);
        const float r = two_pi * fc * dtj;
        const float a = r / (r + 1.0f);
        const float xnew = xh[c] + a * (m[c] - xh[c]);
        xh[c] = xnew;
        dxh[c] = dx;
        out[c] = xnew;
    }
    last = tick;
    return true;
}
