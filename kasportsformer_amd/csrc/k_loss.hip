// The reference's complete seven-term training loss and its gradient in one launch per clip batch (utils/loss_calc.py:6-94 combined as
// train_and_evaluate_sp.py:216-220 spells out `loss_total_complete`):
//   L = mpjpe + l_n n_mpjpe + l_v velocity + l_var limb_len_var + l_len limb_len + l_cs cos_simi + l_cv cos_simi_velocity.
// k_loss7: one workgroup per clip; k_loss7_finish: one workgroup that adds the clips in a fixed order.  fp32 throughout, no atomics, every sum formed in an
// order that does not depend on scheduling (a thread's own loop, a fixed tree over waves, fixed tables) -- dP feeds the whole backward.
//
// Bit contract with k_loss3 (k_misc.hip): the three old terms and their gradient contributions are k_loss3's expressions in k_loss3's order, the extras are
// added to gr[] after them and skipped when their lambdas are 0.f, so with the four new lambdas zero dP and losses[0..3] are kasf_loss3's bits.
//
// Stages ("seven-term loss"): nothing per (frame, limb) is kept in LDS but the two angle arrays and one byte of L1 signs per (frame, angle);
// limb vectors, lengths and cosines are recomputed from P / Y (L1 / L2 hits) where a later stage needs them:
//   0  per frame: k_loss3's n_mpjpe scale, <p,p> and sum_j u_j . p_j                                        -> sS, sDen, sWt [T]
//   1  per (t, limb): len_p, len_y: sum |len_p - len_y|, per-limb sum over t of len_p (16 columns of a 16 x 16 tree) -> sMean [16]
//      per (t, angle): theta_p, theta_y                                                                     -> sThP, sThY [T][18]
//   2  per (t, limb): sum (len_p - mean)^2;  per (t, angle): sum |theta_p - theta_y|, sum |velocity difference|, both signs -> sSg [T][18] bytes
//   3  per (t, joint): k_loss3's gradient, then the signed sum over the joint's <= 4 incident limbs (fixed table) of the limb's gradient vector, itself
//      the length terms plus a gather over the limb's <= 4 angles (fixed table) of dL/dtheta . dtheta/dc . dc/dlimb;  dP written once
// LDS: 174 bytes per frame + 1.2 KB: 42.5 KB at T = 243, below 64 KB up to KASF_LOSS7_MAX_FRAMES.
#include "common.h"
#include "kernels.h"

#ifndef KASF_DYNAMIC_LDS
#define KASF_DYNAMIC_LDS(name) extern __shared__ float name[]
#endif

namespace {

constexpr int NL = 16, NA = 18;     // limbs, angles (utils/loss_calc.py:33-37, 69-72)

struct LossTables {
    signed char limb[NL][2];         // l_k = x[limb[k][0]] - x[limb[k][1]]
    signed char angle[NA][2];        // the two limbs of angle m
    signed char limb_angle[NL][4];   // the angles limb k takes part in (-1: none), ascending
    signed char limb_other[NL][4];   // ... and the other limb of each
    signed char joint_limb[KASF_J][4];   // the limbs joint j is an end of (-1: none), ascending
    signed char joint_sign[KASF_J][4];   // +1: j is the limb's first joint, -1: its second
};

constexpr LossTables make_loss_tables() {
    LossTables t{};
    const int limbs[NL][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 4}, {4, 5}, {5, 6}, {0, 7}, {7, 8}, {8, 9}, {9, 10}, {8, 11}, {11, 12}, {12, 13}, {8, 14}, {14, 15},
                              {15, 16}};
    const int angles[NA][2] = {{0, 3}, {0, 6}, {3, 6}, {0, 1}, {1, 2}, {3, 4}, {4, 5}, {6, 7}, {7, 10}, {7, 13}, {8, 13}, {10, 13}, {7, 8}, {8, 9}, {10, 11},
                               {11, 12}, {13, 14}, {14, 15}};
    for (int k = 0; k < NL; ++k) {
        t.limb[k][0] = (signed char)limbs[k][0];
        t.limb[k][1] = (signed char)limbs[k][1];
        int n = 0;
        for (int e = 0; e < 4; ++e) { t.limb_angle[k][e] = -1; t.limb_other[k][e] = 0; }
        for (int m = 0; m < NA; ++m)
            for (int r = 0; r < 2; ++r)
                if (angles[m][r] == k) { t.limb_angle[k][n] = (signed char)m; t.limb_other[k][n] = (signed char)angles[m][1 - r]; ++n; }
    }
    for (int m = 0; m < NA; ++m) { t.angle[m][0] = (signed char)angles[m][0]; t.angle[m][1] = (signed char)angles[m][1]; }
    for (int j = 0; j < KASF_J; ++j) {
        int n = 0;
        for (int e = 0; e < 4; ++e) { t.joint_limb[j][e] = -1; t.joint_sign[j][e] = 0; }
        for (int k = 0; k < NL; ++k)
            for (int r = 0; r < 2; ++r)
                if (limbs[k][r] == j) { t.joint_limb[j][n] = (signed char)k; t.joint_sign[j][n] = (signed char)(r == 0 ? 1 : -1); ++n; }
    }
    return t;
}
constexpr int max_fanout(bool joints) {
    const int limbs[NL][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 4}, {4, 5}, {5, 6}, {0, 7}, {7, 8}, {8, 9}, {9, 10}, {8, 11}, {11, 12}, {12, 13}, {8, 14}, {14, 15},
                              {15, 16}};
    const int angles[NA][2] = {{0, 3}, {0, 6}, {3, 6}, {0, 1}, {1, 2}, {3, 4}, {4, 5}, {6, 7}, {7, 10}, {7, 13}, {8, 13}, {10, 13}, {7, 8}, {8, 9}, {10, 11},
                               {11, 12}, {13, 14}, {14, 15}};
    int worst = 0;
    for (int i = 0; i < (joints ? KASF_J : NL); ++i) {
        int n = 0;
        if (joints) { for (int k = 0; k < NL; ++k) n += (limbs[k][0] == i) + (limbs[k][1] == i); }
        else { for (int m = 0; m < NA; ++m) n += (angles[m][0] == i) + (angles[m][1] == i); }
        worst = n > worst ? n : worst;
    }
    return worst;
}
static_assert(max_fanout(true) == 4 && max_fanout(false) == 4, "the gather tables hold four entries per row");

__constant__ const LossTables kTab = make_loss_tables();

// acos(clamp(c, -1 + 1e-7, 1 - 1e-7)) with the two bounds rounded to fp32, as torch clamps an fp32 tensor with Python floats
#define KASF_COS_LO ((float)(-1.0 + 1e-7))
#define KASF_COS_HI ((float)(1.0 - 1e-7))
#define KASF_COS_EPS 1e-8f         // torch 2.x cosine_similarity: each vector is divided by max(|v|, 1e-8)

struct Loss7Lambdas { float n, v, var, len, cs, cv; };

__device__ __forceinline__ float len3(float a, float b, float c) { return sqrtf(a * a + b * b + c * c); }
__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }        // torch: sign(0) = 0
__device__ __forceinline__ unsigned sign_code(float d) { return d > 0.f ? 2u : (d < 0.f ? 0u : 1u); }     // sign + 1

// x: one clip [T][17][3]
__device__ __forceinline__ void limb_vec(const float* __restrict__ x, int t, int k, float (&l)[3]) {
    const float* a = x + (t * KASF_J + kTab.limb[k][0]) * 3;
    const float* b = x + (t * KASF_J + kTab.limb[k][1]) * 3;
    l[0] = a[0] - b[0]; l[1] = a[1] - b[1]; l[2] = a[2] - b[2];
}
__device__ __forceinline__ float limb_len(const float* __restrict__ x, int t, int k) {
    float l[3];
    limb_vec(x, t, k, l);
    return len3(l[0], l[1], l[2]);
}
// u = l / max(|l|, eps); returns |l|
__device__ __forceinline__ float limb_unit(const float* __restrict__ x, int t, int k, float (&u)[3]) {
    limb_vec(x, t, k, u);
    const float len = len3(u[0], u[1], u[2]), n = fmaxf(len, KASF_COS_EPS);
    u[0] /= n; u[1] /= n; u[2] /= n;
    return len;
}
__device__ __forceinline__ float dot3(const float (&u)[3], const float (&v)[3]) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }
__device__ __forceinline__ float angle_theta(const float* __restrict__ x, int t, int m) {
    float u[3], v[3];
    limb_unit(x, t, kTab.angle[m][0], u);
    limb_unit(x, t, kTab.angle[m][1], v);
    return acosf(fminf(fmaxf(dot3(u, v), KASF_COS_LO), KASF_COS_HI));
}

struct Loss7Grad {
    const float* p; const float* y;      // the clip
    const float* mean;                   // [16] mean over t of len_p
    const unsigned char* sg;             // [T][18]: bits 0-1 sign(theta_p - theta_y) + 1, bits 2-3 sign(velocity difference t -> t + 1) + 1
    int T;
    float c_var, c_len, c_cs, c_cv;      // lambda / count of each term (0: the term is skipped)
};

// dL/dtheta_p[t][m] of the two angle terms
__device__ __forceinline__ float angle_dtheta(const Loss7Grad& g, int t, int m) {
    float d = 0.f;
    if (g.c_cs != 0.f) d += g.c_cs * ((float)(g.sg[t * NA + m] & 3u) - 1.f);
    if (g.c_cv != 0.f) {
        if (t > 0) d += g.c_cv * ((float)((g.sg[(t - 1) * NA + m] >> 2) & 3u) - 1.f);
        if (t < g.T - 1) d -= g.c_cv * ((float)((g.sg[t * NA + m] >> 2) & 3u) - 1.f);
    }
    return d;
}

// G = dL/dl_k[t] of the four limb terms
__device__ __forceinline__ void limb_grad(const Loss7Grad& g, int t, int k, float (&G)[3]) {
    float l[3];
    limb_vec(g.p, t, k, l);
    const float len = len3(l[0], l[1], l[2]);
    G[0] = G[1] = G[2] = 0.f;
    if ((g.c_var != 0.f || g.c_len != 0.f) && len > 0.f) {      // the gradient of a norm at the zero vector is zero
        float s = 0.f;
        if (g.c_var != 0.f) s += g.c_var * (len - g.mean[k]);
        if (g.c_len != 0.f) s += g.c_len * sign_of(len - limb_len(g.y, t, k));
#pragma unroll
        for (int d = 0; d < 3; ++d) G[d] += s * l[d] / len;
    }
    if (g.c_cs != 0.f || g.c_cv != 0.f) {
        const float n = fmaxf(len, KASF_COS_EPS);
        const float u[3] = {l[0] / n, l[1] / n, l[2] / n};
        for (int e = 0; e < 4; ++e) {
            const int m = kTab.limb_angle[k][e];
            if (m < 0) break;
            const float dth = angle_dtheta(g, t, m);
            if (dth == 0.f) continue;
            float v[3];
            limb_unit(g.p, t, kTab.limb_other[k][e], v);
            const float c = dot3(u, v);               // the products commute: the forward's bits whichever of the two limbs this one is
            if (c < KASF_COS_LO || c > KASF_COS_HI) continue;      // no gradient through clamp outside its closed range
            const float dc = -dth / sqrtf(1.f - c * c);
            // d(u . v)/dl with u = l / max(|l|, eps): (v - c u) / |l| above eps; below it the divisor is the constant eps and u' = I / eps
#pragma unroll
            for (int d = 0; d < 3; ++d) G[d] += len >= KASF_COS_EPS ? dc * (v[d] - c * u[d]) / len : dc * v[d] / KASF_COS_EPS;
        }
    }
}

__global__ __launch_bounds__(256) void k_loss7(const float* __restrict__ P, const float* __restrict__ Y, float* __restrict__ dP, float* __restrict__ losses,
                                               int B, int T, Loss7Lambdas lam, float gscale) {
    KASF_DYNAMIC_LDS(sm);
    float* sS = sm;            // [T] scale
    float* sDen = sS + T;      // [T]
    float* sWt = sDen + T;     // [T] sum_j u_j . p_j
    float* sThP = sWt + T;     // [T][18]
    float* sThY = sThP + T * NA;
    unsigned char* sSg = reinterpret_cast<unsigned char*>(sThY + T * NA);      // [T][18]
    __shared__ float sL[4][7];
    __shared__ float sRed[256];
    __shared__ float sMean[NL];
    const int b = blockIdx.x;
    const float lam_n = lam.n, lam_v = lam.v;
    const float* p = P + (int64_t)b * T * 51;
    const float* y = Y + (int64_t)b * T * 51;
    float* dp = dP + (int64_t)b * T * 51;
    // ---- stage 0: k_loss3's per-frame pass ----
    for (int t = threadIdx.x; t < T; t += 256) {
        float den = 0.f, num = 0.f;
        for (int k = 0; k < 51; ++k) { den += p[t * 51 + k] * p[t * 51 + k]; num += y[t * 51 + k] * p[t * 51 + k]; }
        sDen[t] = den;
        const float s = num / den;
        sS[t] = s;
        float wt = 0.f;                                  // sum over the frame's joints of u_j . p_j, u_j = e_j / |e_j|, e_j = s p_j - y_j
        for (int j = 0; j < KASF_J; ++j) {
            const int it = t * KASF_J + j;
            const float e0 = s * p[it * 3] - y[it * 3], e1 = s * p[it * 3 + 1] - y[it * 3 + 1], e2 = s * p[it * 3 + 2] - y[it * 3 + 2];
            const float n = len3(e0, e1, e2);
            if (n > 0.f) wt += (e0 * p[it * 3] + e1 * p[it * 3 + 1] + e2 * p[it * 3 + 2]) / n;
        }
        sWt[t] = wt;
    }
    // ---- stage 1: limb lengths (256 = 16 x 16: a thread stays on limb threadIdx.x & 15) and angles ----
    float a_var = 0.f, a_len = 0.f, a_cs = 0.f, a_cv = 0.f;
    {
        float own = 0.f;
        for (int it = threadIdx.x; it < T * NL; it += 256) {
            const int t = it >> 4, k = it & 15;
            const float lp = limb_len(p, t, k);
            own += lp;
            a_len += fabsf(lp - limb_len(y, t, k));
        }
        sRed[threadIdx.x] = own;
    }
    for (int it = threadIdx.x; it < T * NA; it += 256) {
        const int t = it / NA, m = it - t * NA;
        sThP[it] = angle_theta(p, t, m);
        sThY[it] = angle_theta(y, t, m);
    }
    __syncthreads();
    if (threadIdx.x < NL) {
        float s = 0.f;
        for (int r = 0; r < 16; ++r) s += sRed[r * 16 + threadIdx.x];
        sMean[threadIdx.x] = s / (float)T;
    }
    __syncthreads();
    // ---- stage 2: the variance's squares, the angle terms and their signs ----
    for (int it = threadIdx.x; it < T * NL; it += 256) {
        const float dev = limb_len(p, it >> 4, it & 15) - sMean[it & 15];
        a_var += dev * dev;
    }
    for (int it = threadIdx.x; it < T * NA; it += 256) {
        const int t = it / NA;
        const float d = sThP[it] - sThY[it];
        a_cs += fabsf(d);
        unsigned code = sign_code(d);
        if (t < T - 1) {
            const float w = (sThP[it + NA] - sThP[it]) - (sThY[it + NA] - sThY[it]);
            a_cv += fabsf(w);
            code |= sign_code(w) << 2;
        }
        sSg[it] = (unsigned char)code;
    }
    __syncthreads();
    // ---- stage 3: k_loss3's two loops, the extras added to gr[] behind its three terms ----
    const float n1 = (float)B * T * KASF_J, n3 = (float)B * (T - 1) * KASF_J;
    Loss7Grad g;
    g.p = p; g.y = y; g.mean = sMean; g.sg = sSg; g.T = T;
    g.c_var = (lam.var != 0.f && T > 1) ? lam.var * 2.f / ((float)B * NL * (T - 1)) : 0.f;
    g.c_len = lam.len != 0.f ? lam.len / ((float)B * T * NL) : 0.f;
    g.c_cs = lam.cs != 0.f ? lam.cs / ((float)B * T * NA) : 0.f;
    g.c_cv = (lam.cv != 0.f && T > 1) ? lam.cv / ((float)B * (T - 1) * NA) : 0.f;
    const bool extras = g.c_var != 0.f || g.c_len != 0.f || g.c_cs != 0.f || g.c_cv != 0.f;
    float l1 = 0.f, l2 = 0.f, l3 = 0.f;
    for (int it = threadIdx.x; it < T * KASF_J; it += 256) {
        const int t = it / KASF_J;
        const float s = sS[t];
        const float e0 = s * p[it * 3] - y[it * 3], e1 = s * p[it * 3 + 1] - y[it * 3 + 1], e2 = s * p[it * 3 + 2] - y[it * 3 + 2];
        l2 += len3(e0, e1, e2);
    }
    for (int it = threadIdx.x; it < T * KASF_J; it += 256) {
        const int t = it / KASF_J;
        float gr[3] = {0.f, 0.f, 0.f};
        const float pv[3] = {p[it * 3], p[it * 3 + 1], p[it * 3 + 2]}, yv[3] = {y[it * 3], y[it * 3 + 1], y[it * 3 + 2]};
        {   // mpjpe
            const float e0 = pv[0] - yv[0], e1 = pv[1] - yv[1], e2 = pv[2] - yv[2], n = len3(e0, e1, e2);
            l1 += n;
            if (n > 0.f) { gr[0] += e0 / n / n1; gr[1] += e1 / n / n1; gr[2] += e2 / n / n1; }
        }
        {   // n_mpjpe: e = s p - y, s = <y,p>/<p,p> per frame; d/dp_k = s u_k + (sum_j u_j.p_j) (y_k - 2 s p_k) / <p,p>
            const float s = sS[t], wt = sWt[t], den = sDen[t];
            const float e0 = s * pv[0] - yv[0], e1 = s * pv[1] - yv[1], e2 = s * pv[2] - yv[2], n = len3(e0, e1, e2);
            const float u[3] = {n > 0.f ? e0 / n : 0.f, n > 0.f ? e1 / n : 0.f, n > 0.f ? e2 / n : 0.f};
#pragma unroll
            for (int d = 0; d < 3; ++d) gr[d] += lam_n * (s * u[d] + wt * (yv[d] - 2.f * s * pv[d]) / den) / n1;
        }
        if (T > 1) {   // velocity
            if (t < T - 1) {
                const int nx = it + KASF_J;
                const float v0 = (p[nx * 3] - pv[0]) - (y[nx * 3] - yv[0]), v1 = (p[nx * 3 + 1] - pv[1]) - (y[nx * 3 + 1] - yv[1]),
                            v2 = (p[nx * 3 + 2] - pv[2]) - (y[nx * 3 + 2] - yv[2]);
                const float n = len3(v0, v1, v2);
                l3 += n;
                if (n > 0.f) { gr[0] -= lam_v * v0 / n / n3; gr[1] -= lam_v * v1 / n / n3; gr[2] -= lam_v * v2 / n / n3; }
            }
            if (t > 0) {
                const int pr = it - KASF_J;
                const float v0 = (pv[0] - p[pr * 3]) - (yv[0] - y[pr * 3]), v1 = (pv[1] - p[pr * 3 + 1]) - (yv[1] - y[pr * 3 + 1]),
                            v2 = (pv[2] - p[pr * 3 + 2]) - (yv[2] - y[pr * 3 + 2]);
                const float n = len3(v0, v1, v2);
                if (n > 0.f) { gr[0] += lam_v * v0 / n / n3; gr[1] += lam_v * v1 / n / n3; gr[2] += lam_v * v2 / n / n3; }
            }
        }
        if (extras) {   // the joint's incident limbs in table order: x[a] takes +G, x[b] takes -G
            const int j = it - t * KASF_J;
            for (int e = 0; e < 4; ++e) {
                const int k = kTab.joint_limb[j][e];
                if (k < 0) break;
                float G[3];
                limb_grad(g, t, k, G);
                const float sg = (float)kTab.joint_sign[j][e];
                gr[0] += sg * G[0]; gr[1] += sg * G[1]; gr[2] += sg * G[2];
            }
        }
        dp[it * 3] = gr[0] * gscale; dp[it * 3 + 1] = gr[1] * gscale; dp[it * 3 + 2] = gr[2] * gscale;
    }
    l1 = reduce64(l1); l2 = reduce64(l2); l3 = reduce64(l3);
    a_var = reduce64(a_var); a_len = reduce64(a_len); a_cs = reduce64(a_cs); a_cv = reduce64(a_cv);
    if ((threadIdx.x & 63) == 0) {
        float* r = sL[threadIdx.x >> 6];
        r[0] = l1; r[1] = l2; r[2] = l3; r[3] = a_var; r[4] = a_len; r[5] = a_cs; r[6] = a_cv;
    }
    __syncthreads();
    if (threadIdx.x < 7) losses[8 + 8 * b + threadIdx.x] = (sL[0][threadIdx.x] + sL[1][threadIdx.x]) + (sL[2][threadIdx.x] + sL[3][threadIdx.x]);
    if (threadIdx.x == 7) losses[8 + 8 * b + 7] = 0.f;
}

// losses[0..7] = {total, mpjpe, n_mpjpe, velocity, limb_len_var, limb_len, cos_simi, cos_simi_velocity} from the per-clip sums at losses[8 + 8 b + k]
// (k = the part's index - 1): one workgroup, fixed order
__global__ __launch_bounds__(256) void k_loss7_finish(float* __restrict__ losses, int B, int T, Loss7Lambdas lam) {
    __shared__ float sP[256][7];
    float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < B; b += 256)
#pragma unroll
        for (int k = 0; k < 7; ++k) a[k] += losses[8 + 8 * b + k];
#pragma unroll
    for (int k = 0; k < 7; ++k) sP[threadIdx.x][k] = a[k];
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (threadIdx.x < h)
#pragma unroll
            for (int k = 0; k < 7; ++k) sP[threadIdx.x][k] += sP[threadIdx.x + h][k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float n1 = (float)B * T * KASF_J, n3 = (float)B * (T - 1) * KASF_J;
        const float m1 = sP[0][0] / n1, m2 = sP[0][1] / n1, m3 = T > 1 ? sP[0][2] / n3 : 0.f;
        const float m4 = T > 1 ? sP[0][3] / ((float)B * NL * (T - 1)) : 0.f, m5 = sP[0][4] / ((float)B * T * NL), m6 = sP[0][5] / ((float)B * T * NA),
                    m7 = T > 1 ? sP[0][6] / ((float)B * (T - 1) * NA) : 0.f;
        float total = m1 + lam.n * m2 + lam.v * m3;
        if (lam.var != 0.f) total += lam.var * m4;
        if (lam.len != 0.f) total += lam.len * m5;
        if (lam.cs != 0.f) total += lam.cs * m6;
        if (lam.cv != 0.f) total += lam.cv * m7;
        losses[0] = total;
        losses[1] = m1; losses[2] = m2; losses[3] = m3; losses[4] = m4; losses[5] = m5; losses[6] = m6; losses[7] = m7;
    }
}

}  // namespace

int64_t kasf_loss7_lds_bytes(int T) { return (int64_t)T * ((3 + 2 * NA) * (int64_t)sizeof(float) + NA); }

void kasf_launch_loss7(hipStream_t s, const float* pred, const float* tgt, float* dpred, float* losses, int B, int T, const float* lambdas, float grad_scale) {
    const Loss7Lambdas lam = {lambdas[0], lambdas[1], lambdas[2], lambdas[3], lambdas[4], lambdas[5]};
    hipLaunchKernelGGL(k_loss7, dim3(B), dim3(256), (size_t)kasf_loss7_lds_bytes(T), s, pred, tgt, dpred, losses, B, T, lam, grad_scale);
    hipLaunchKernelGGL(k_loss7_finish, dim3(1), dim3(256), 0, s, losses, B, T, lam);
}
