// GCN mixer (reference: modules/graph.py:19-134), split at the BatchNorm batch-statistics barrier:
//   uv = LN(x) [U|V]^T + b                       (k_linear, writes xn = LN(x))
//   y  = A_hat . V(xn) + U(xn)                   k_gcn_agg_{spatial,temporal}  (+ per-node sum / sum-of-squares)
//   coef = BatchNorm scale/shift per node        k_bn_finalize               (+ running statistics, graph.py:37)
//   out = x + ls1 * relu(xn + y*scale + shift)   k_gcn_apply                 (graph.py:128-129, KASportsFormer.py:109)
// spatial : fixed skeleton adjacency (graph.py:16-17,52-61), D^-1/2 A D^-1/2, nodes = joints, BN channel = joint
// temporal: per (b, joint) track, S = xn xn^T, threshold = 4th largest per row, A = (S >= thr) (ties kept,
//           graph.py:104-112), D from row sums (graph.py:77-90), BN channel = frame.  The adjacency is a
//           comparison result and carries no gradient; its bit mask is stored for the backward pass.
#include "common.h"
#include "kernels.h"

namespace {

// skeleton neighbours (graph.py:16-17) and D^-1/2 A D^-1/2 coefficients, filled by the host at load time
struct SkelTable { int nb[KASF_J][4]; float coef[KASF_J][4]; };
__constant__ SkelTable c_skel;
// The table as the spatial kernels read it (round 5): in LDS, and with a missing neighbour (nb < 0) replaced by the joint itself at coefficient 0, so that the gather needs no branch.
struct SkelLds { int nb[KASF_J][4]; __attribute__((aligned(16))) float coef[KASF_J][4]; };
__device__ __forceinline__ void skel_to_lds(SkelLds& d) {            // the caller's next __syncthreads() publishes it
    for (int k = threadIdx.x; k < KASF_J * 4; k += blockDim.x) {
        const int i = k >> 2, e = k & 3, nb = c_skel.nb[i][e];
        d.nb[i][e] = nb >= 0 ? nb : i;
        d.coef[i][e] = nb >= 0 ? c_skel.coef[i][e] : 0.0f;
    }
}

constexpr int COEF_LD = 8;      // per node: scale, shift, mean, rstd, c1, c2, -, -
constexpr int MASK_W = 3;       // 32-bit words per adjacency row of the T <= 96 instantiations (any T: kasf_gcn_mask_words)
constexpr int SX_LD = 132;      // padded fp32 row of the temporal tiles

// Batch statistics cross workgroups through an EXACT accumulator (round 5): every per-workgroup partial sum is split into 52-bit pieces of a fixed-point
// number and added with 64-bit INTEGER atomics -- integer addition is associative, so the total does not depend on the order in which workgroups arrive
// (the fp64 atomic adds of rounds 1-4 were order-dependent below 1e-15 relative: the one stated exception to bit-reproducible gradients, include/kasf.h).
// One statistic = KASF_STAT_WORDS int64 words: word k (k < 4) counts units of 2^(KASF_STAT_E0 + 52 k), i.e. bits 2^-110 .. 2^98 (partials are fp32 sums: their 24-bit
// mantissas straddle at most two words; what lies below 2^-110 is dropped, toward -inf); 12 spare bits per word hold the carries of up to 2^11 additions
// (grids are capped at 1,024 workgroups, 256 per slot); word 4 is a poison flag (a non-finite or >= 2^97 partial: readers return NaN, as the fp64 sum did).
// KASF_STAT_SLOTS copies ([slot][2 x 256 nodes][words], slot = workgroup index mod slots) because a thousand workgroups each ending in atomics on the same
// 34..162 addresses serialise at the memory side (44 us for the spatial aggregate with one copy, 24 us without the atomics); readers add the copies up.
constexpr int KASF_STAT_E0 = -110;
__device__ __forceinline__ double stat_sum(const double* stats, int idx) {
    const long long* w = reinterpret_cast<const long long*>(stats);
    long long acc[KASF_STAT_WORDS];
#pragma unroll
    for (int k = 0; k < KASF_STAT_WORDS; ++k) acc[k] = 0;
#pragma unroll
    for (int sl = 0; sl < KASF_STAT_SLOTS; ++sl)
#pragma unroll
        for (int k = 0; k < KASF_STAT_WORDS; ++k) acc[k] += w[((int64_t)sl * KASF_STAT_LD + idx) * KASF_STAT_WORDS + k];
    if (acc[KASF_STAT_WORDS - 1] != 0) return __builtin_nan("");
    double v = 0.0;                              // most significant word first; every word is an integer scaled by an exact power of two (its conversion to double rounds once above 2^53, always the same way), the three additions round deterministically: the total does not depend on arrival order
#pragma unroll
    for (int k = KASF_STAT_WORDS - 2; k >= 0; --k) v += ldexp((double)acc[k], KASF_STAT_E0 + 52 * k);
    return v;
}
__device__ __forceinline__ void stat_add(double* slot, int idx, double v) {
    unsigned long long* w = reinterpret_cast<unsigned long long*>(slot) + (int64_t)idx * KASF_STAT_WORDS;
    if (v == 0.0) return;
    if (!(fabs(v) < 0x1p97)) { atomicOr(w + KASF_STAT_WORDS - 1, 1ull); return; }      // NaN, inf, or beyond the accumulator's range
    int e;
    const double m = frexp(v, &e);               // v = m 2^e, 1/2 <= |m| < 1
    unsigned long long a = (unsigned long long)ldexp(fabs(m), 53);                     // 53-bit integer mantissa: |v| = a 2^(e - 53)
    int p = e - 53 - KASF_STAT_E0;               // position of a's lowest bit above the accumulator's lowest
    const bool neg = v < 0.0;
    if (p < 0) {                                 // bits below 2^E0: dropped toward -inf (floor of the signed value)
        const int sh = -p;
        if (sh >= 54) { a = neg ? 1 : 0; }
        else { const unsigned long long lost = a & ((1ull << sh) - 1); a >>= sh; if (neg && lost) a += 1; }
        p = 0;
        if (a == 0) return;
    }
    const int k = p / 52, r = p % 52;
    const unsigned long long lo = (a & ((1ull << (52 - r)) - 1)) << r, hi = a >> (52 - r);      // lo < 2^52 in word k, hi < 2^(r+2) in word k + 1 (k + 1 <= 3 below 2^97)
    if (lo) atomicAdd(w + k, neg ? (0ull - lo) : lo);
    if (hi) atomicAdd(w + k + 1, neg ? (0ull - hi) : hi);
}
__device__ __forceinline__ double* stat_slot(double* stats) { return stats + (int64_t)(blockIdx.x % KASF_STAT_SLOTS) * KASF_STAT_LD * KASF_STAT_WORDS; }

// 32-bit token arithmetic (the engine bounds M * 16 below 2^31): a 64-bit divide by 17 is ~40 instructions per lane, paid by all 16 lanes of a token
__device__ __forceinline__ int node_of(int tok, int T, int mode) { return mode == 0 ? tok % KASF_J : (tok / KASF_J) % T; }

// ------------------------------------------------------------------ spatial aggregate (elementwise + 4-neighbour gather)
template <typename T>
__global__ __launch_bounds__(256) void k_gcn_agg_spatial(const T* __restrict__ uv, T* __restrict__ y, double* __restrict__ stats, int64_t M) {
    // one private row of node sums per 16-lane group, touched by that group's lane 0 only (in program order), and a fixed-order sum over the 16 rows:
    // the workgroup's contribution does not depend on wave scheduling (LDS float atomics from several waves would)
    __shared__ float sStat[16][KASF_J * 2];
    __shared__ SkelLds sSk;
    for (int k = threadIdx.x; k < 16 * KASF_J * 2; k += 256) (&sStat[0][0])[k] = 0.f;
    skel_to_lds(sSk);
    __syncthreads();
    const int sub = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int n_items = (int)(M * 16);
    for (int item = blockIdx.x * 256 + threadIdx.x; item < n_items; item += gridDim.x * 256) {
        const int tk = item >> 4, fr = (tk / KASF_J) * KASF_J;
        const int64_t tok = tk, frame0 = fr;
        const int i = tk - fr;
        // Round 5: the four neighbour rows are requested TOGETHER with the token's own -- a missing neighbour reads the token's own V row with coefficient 0 -- instead of one
        // guarded load after another (hipcc turns `if (nb >= 0) load` into a branch with a full wait per neighbour, and the per-lane table lookups in constant memory were
        // vector loads of their own in front of each): five independent 16-byte loads per lane in flight, the table in LDS.
        const f32x4 cf = *reinterpret_cast<const f32x4*>(sSk.coef[i]);
        const int nbs[4] = {sSk.nb[i][0], sSk.nb[i][1], sSk.nb[i][2], sSk.nb[i][3]};
        float acc[8], v[4][8];
        load8(uv + tok * 256 + sub * 8, acc);                        // U
#pragma unroll
        for (int e = 0; e < 4; ++e) load8(uv + (frame0 + nbs[e]) * 256 + 128 + sub * 8, v[e]);      // V of the neighbour joints
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float c = cf[e];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += c * v[e][k];
        }
        store8(y + tok * 128 + sub * 8, acc);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float r = to_f(from_f<T>(acc[k])); s1 += r; s2 += r * r; }   // statistics of the stored value
        s1 = reduce16(s1);
        s2 = reduce16(s2);
        if (sub == 0) { sStat[rl][i * 2] += s1; sStat[rl][i * 2 + 1] += s2; }
    }
    __syncthreads();
    if (threadIdx.x < KASF_J * 2) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sStat[k][threadIdx.x];
        stat_add(stat_slot(stats), threadIdx.x, (double)t);
    }
}

// ------------------------------------------------------------------ temporal aggregate: persistent workgroups, one (b, joint) track at a time
// S = xn xn^T runs on the matrix cores (bf16: v_mfma_f32_16x16x32_bf16 on the stored bf16 rows, exact products, fp32 accumulate;
// fp32 mode: the exact v_mfma_f32_16x16x4_f32 chain).  Both operands are the SAME rows in the same k order, so S is bitwise symmetric.
// BatchNorm sums are kept in LDS across all tracks of the workgroup and leave it as ONE fp64 atomic per frame at the end.
template <int L> constexpr int agg_lp() { return (L + 15) / 16 * 16; }
// LDS: the similarity matrix and the V rows are never live together (S dies with the top-4 scan, V is first read by the aggregation), so they share one
// region: 24.5 + 26.6 + 2 KB at T = 81 in bf16 -- THREE workgroups per CU where round 3's 78 KB allowed two (55 % of that launch's wave-cycles were waits).
template <int L> constexpr int agg_ss_ld() { return (L | 1) + 1 + ((((L | 1) + 1) % 32 == 0) ? 2 : 0); }     // row stride of S in floats: >= L, even, not a multiple of 32
template <typename T, int L> constexpr size_t agg_region2() {
    return (size_t)L * agg_ss_ld<L>() * sizeof(float) > (size_t)L * 128 * sizeof(T) ? (size_t)L * agg_ss_ld<L>() * sizeof(float) : (size_t)L * 128 * sizeof(T);
}
template <typename T, int L>
__global__ __launch_bounds__(256, (sizeof(T) == 2 && L == 81) ? 3 : 1) void k_gcn_agg_temporal(const T* __restrict__ uv, const T* __restrict__ xn, T* __restrict__ y,
                                                          uint32_t* __restrict__ mask, double* __restrict__ stats, int Tn, int kth, int n_tracks) {
    constexpr int LP = agg_lp<L>(), NTL = LP / 16, EPC = Tile<T>::EPC, CPR = Tile<T>::CPR, SS = agg_ss_ld<L>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* sX = reinterpret_cast<T*>(smem);                 // [LP][128] swizzled tile, LN(x) rows of the track (rows >= L stay zero)
    T* sV = sX + LP * 128;                              // [L][128]  V rows        } one region: S until the scan is done,
    float* sS = reinterpret_cast<float*>(sV);           // [L][SS]   similarity    } V from then on
    float* sDinv = reinterpret_cast<float*>(reinterpret_cast<char*>(sV) + agg_region2<T, L>());   // [L]
    float* sStat = sDinv + L;                           // [L][2]    running BatchNorm sums of this workgroup
    uint32_t* sMask = reinterpret_cast<uint32_t*>(sStat + 2 * L);   // [L][MASK_W]
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    for (int idx = threadIdx.x; idx < (LP - L) * CPR; idx += 256) {
        const int r = L + idx / CPR, ch = idx % CPR;
        float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (EPC == 8) tile_store8(sX, r, ch * 8, z);
        else { float z4[4] = {0.f, 0.f, 0.f, 0.f}; store4(sX + Tile<float>::chunk_off(r, ch), z4); }
    }
    if (threadIdx.x < 2 * L) sStat[threadIdx.x] = 0.f;
    // The LN(x) and V chunks of a track (raw 16-byte copies, no conversion on the way in) are requested ONE TRACK AHEAD (round 4): the loads of track n + 1
    // go out as soon as track n's V image is in LDS and land under its aggregation and the next track's ... nothing waits for them at the top of a track.
    // (Round 2 issued them at the top of their own track: one exposed HBM round trip per track, 55 % of the wave-cycles of the T = 81 launch spent waiting.)
    constexpr int NI = (L * CPR + 255) / 256, NI4 = (L * 16 + 255) / 256;
    f32x4 rx[NI], rv[NI];
    Raw8<T> ru[NI4];
    auto fetch = [&](int G) {
        const int b = G / KASF_J, j = G % KASF_J;
        auto tok = [&](int r) { return ((int64_t)b * Tn + r) * KASF_J + j; };
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const int idx = threadIdx.x + 256 * k;
            if (idx < L * CPR) {
                const int r = idx / CPR, ch = idx % CPR;
                rx[k] = *reinterpret_cast<const f32x4*>(xn + tok(r) * 128 + ch * EPC);
                rv[k] = *reinterpret_cast<const f32x4*>(uv + tok(r) * 256 + 128 + ch * EPC);
            }
        }
    };
    // the U chunks are only needed by the aggregation at the END of their own track: requested at its top (two phases of cover), not a track ahead
    // (a second register image of them is what made the T = 81 kernel spill at three workgroups per CU)
    auto fetch_u = [&](int G) {
        const int b = G / KASF_J, j = G % KASF_J;
#pragma unroll
        for (int k = 0; k < NI4; ++k) {
            const int idx = threadIdx.x + 256 * k;
            if (idx < L * 16) ru[k].load(uv + (((int64_t)b * Tn + (idx >> 4)) * KASF_J + j) * 256 + (idx & 15) * 8);
        }
    };
    if ((int)blockIdx.x < n_tracks) fetch(blockIdx.x);
    for (int G = blockIdx.x; G < n_tracks; G += gridDim.x) {
        const int b = G / KASF_J, j = G % KASF_J;
        auto tok = [&](int r) { return ((int64_t)b * Tn + r) * KASF_J + j; };
        __syncthreads();                                // previous track fully consumed (and the zero fill / sStat init visible)
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const int idx = threadIdx.x + 256 * k;
            if (idx < L * CPR) {
                const int r = idx / CPR, ch = idx % CPR;
                *reinterpret_cast<f32x4*>(sX + Tile<T>::chunk_off(r, ch)) = rx[k];
            }
        }
        fetch_u(G);
        __syncthreads();
        for (int t = w; t < NTL * NTL; t += 4) {        // 16x16 tiles of S over the 4 waves
            const int tn = t / NTL, tm = t % NTL;
            f32x4 acc[1][1];
            zero_acc(acc);
            mma_k128<1, 1>(sX, tn * 16, sX, tm * 16, acc);
            const int r = tm * 16 + li;                 // acc[r4] = S[row r][col tn*16 + 4*lg + r4]
            if (r < L) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = tn * 16 + 4 * lg + q;
                    if (c < L) sS[r * SS + c] = acc[0][0][q];
                }
            }
        }
        __syncthreads();
        // k-th largest per row -> adjacency bits and degree (graph.py:104-112: ties kept).  NL lanes per row, columns interleaved (c = j mod NL): each keeps
        // the four largest of its columns (with multiplicity), merges with the row's other lanes, then sets the mask bits of its own columns; the words are
        // OR-ed across the row's lanes.  A wave holds RW = 64 / NL whole rows and the four waves cover all L rows in ONE pass whenever 4 RW >= L (T = 81:
        // three lanes per row, 21 rows per wave; round 2's four lanes per row needed a second pass in which 17 of 64 row slots were live).
        constexpr int NL = L <= 64 ? 4 : (L <= 84 ? 3 : 4), RW = 64 / NL;
        for (int r0 = 0; r0 < L; r0 += 4 * RW) {
            const int slot = lane / NL, j = lane - slot * NL, base = slot * NL;
            const int r = r0 + w * RW + slot;
            const bool live = slot < RW && r < L;
            float top[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (live) {
                for (int c = j; c < L; c += NL) {
                    float v = sS[r * SS + c];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {          // compare-exchange as max / min (S is finite): two instructions per level
                        const float hi = fmaxf(top[e], v);
                        v = fminf(top[e], v);
                        top[e] = hi;
                    }
                }
            }
            if constexpr (NL == 4) {                         // butterfly: after each step both partners hold the merged four
#pragma unroll
                for (int m = 1; m <= 2; m <<= 1) {
                    float o[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = __shfl_xor(top[e], m);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float v = o[q];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float hi = fmaxf(top[e], v);
                            v = fminf(top[e], v);
                            top[e] = hi;
                        }
                    }
                }
            } else {                                         // three lanes per row: every lane inserts the ORIGINAL fours of the other two, each exactly once
                const float own[4] = {top[0], top[1], top[2], top[3]};
#pragma unroll
                for (int m = 1; m < NL; ++m) {
                    int src = j + m;
                    src = base + (src >= NL ? src - NL : src);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float v = __shfl(own[q], src);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float hi = fmaxf(top[e], v);
                            v = fminf(top[e], v);
                            top[e] = hi;
                        }
                    }
                }
            }
            const float thr = kth <= 1 ? top[0] : (kth == 2 ? top[1] : (kth == 3 ? top[2] : top[3]));
            uint32_t wd[MASK_W] = {0u, 0u, 0u};
            int deg = 0;
            if (live) {
                for (int c = j; c < L; c += NL) {
                    if (sS[r * SS + c] >= thr) { wd[c >> 5] |= 1u << (c & 31); ++deg; }
                }
            }
            uint32_t wo[MASK_W] = {wd[0], wd[1], wd[2]};
            int dsum = deg;
#pragma unroll
            for (int m = 1; m < NL; ++m) {
                int src = j + m;
                src = base + (src >= NL ? src - NL : src);
#pragma unroll
                for (int e = 0; e < MASK_W; ++e) wo[e] |= (uint32_t)__shfl((int)wd[e], src);
                dsum += __shfl(deg, src);
            }
            if (live && j == 0) {
#pragma unroll
                for (int e = 0; e < MASK_W; ++e) { sMask[r * MASK_W + e] = wo[e]; mask[((int64_t)G * L + r) * MASK_W + e] = wo[e]; }
                sDinv[r] = 1.0f / sqrtf((float)dsum);
            }
        }
        __syncthreads();                                // the scan is done with S: its region takes the V rows now, and the NEXT track's loads go out
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const int idx = threadIdx.x + 256 * k;
            if (idx < L * CPR) *reinterpret_cast<f32x4*>(sV + (idx / CPR) * 128 + (idx % CPR) * EPC) = rv[k];
        }
        if (G + (int)gridDim.x < n_tracks) fetch(G + gridDim.x);
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < NI4; ++k4) {
            const int idx = threadIdx.x + 256 * k4;
            if (idx >= L * 16) break;
            const int r = idx >> 4, sub = idx & 15;
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            const float dr = sDinv[r];
            // (tried in round 4: requesting the next neighbour's V chunk and degree one visit ahead -- 117 against 85 us at T = 81: the data-dependent
            //  trip count turns the hand-pipelined form into more branches, not fewer waits)
#pragma unroll
            for (int wi = 0; wi < (L + 31) / 32; ++wi) {
                uint32_t bits = sMask[r * MASK_W + wi];
                while (bits) {                           // visit set bits only (>= 4 neighbours per row, rarely more)
                    const int c = wi * 32 + __builtin_ctz(bits);
                    bits &= bits - 1;
                    const float wgt = dr * sDinv[c];
                    float v[8];
                    load8(sV + c * 128 + sub * 8, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += wgt * v[e];
                }
            }
            float s1 = 0.f, s2 = 0.f, u[8];
            ru[k4].get(u);
#pragma unroll
            for (int e = 0; e < 8; ++e) { acc[e] += u[e]; const float q = to_f(from_f<T>(acc[e])); s1 += q; s2 += q * q; }
            store8(y + tok(r) * 128 + sub * 8, acc);
            s1 = reduce16(s1);
            s2 = reduce16(s2);
            if (sub == 0) { atomicAdd(&sStat[r * 2], s1); atomicAdd(&sStat[r * 2 + 1], s2); }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * L) stat_add(stat_slot(stats), threadIdx.x, (double)sStat[threadIdx.x]);
}

// ------------------------------------------------------------------ BatchNorm1d(num_nodes) + ReLU + layer-scale + residual
// BatchNorm coefficients of one node from the batch sums (training) or the running statistics (evaluation): graph.py:37
__device__ __forceinline__ void bn_node_coef(const double* stats, const float* w, const float* bias, const float* run_mean, const float* run_var, int n,
                                             double count, int training, float& scale, float& shift, float& mean, float& rstd, float& var_unbiased) {
    float var;
    if (training) {
        const double m = stat_sum(stats, 2 * n) / count;
        double v = stat_sum(stats, 2 * n + 1) / count - m * m;
        if (v < 0) v = 0;
        mean = (float)m;
        var = (float)v;
        var_unbiased = (float)(v * count / (count - 1.0));
    } else {
        mean = run_mean[n];
        var = run_var[n];
        var_unbiased = var;
    }
    rstd = 1.0f / sqrtf(var + 1e-5f);
    scale = w[n] * rstd;
    shift = bias[n] - mean * scale;
}

// out = x + ls1 * relu(xn + BN(y)).  Every workgroup derives the per-node affine itself from the (complete) batch sums -- 17 to 81 nodes --
// instead of waiting for a one-workgroup finalize launch; workgroup 0 also publishes the coefficients for the backward pass and updates
// the running statistics.
template <typename T>
__global__ __launch_bounds__(256) void k_gcn_apply(const T* __restrict__ x_in, const T* __restrict__ xn, const T* __restrict__ y,
                                                   const double* __restrict__ stats, const float* __restrict__ bn_w, const float* __restrict__ bn_b,
                                                   float* __restrict__ run_mean, float* __restrict__ run_var, float* __restrict__ coef,
                                                   const float* __restrict__ ls1, T* __restrict__ out, int64_t M, int Tn, int mode, int nodes, double count,
                                                   int training, float momentum) {
    __shared__ float sC[KASF_MAX_NODES][2];
    if ((int)threadIdx.x < nodes) {
        const int n = threadIdx.x;
        float scale, shift, mean, rstd, varu;
        bn_node_coef(stats, bn_w, bn_b, run_mean, run_var, n, count, training, scale, shift, mean, rstd, varu);
        sC[n][0] = scale;
        sC[n][1] = shift;
        if (blockIdx.x == 0) {
            coef[n * COEF_LD + 0] = scale;
            coef[n * COEF_LD + 1] = shift;
            coef[n * COEF_LD + 2] = mean;
            coef[n * COEF_LD + 3] = rstd;
            if (training) {
                run_mean[n] = (1.0f - momentum) * run_mean[n] + momentum * mean;
                run_var[n] = (1.0f - momentum) * run_var[n] + momentum * varu;
            }
        }
    }
    __syncthreads();
    const int sub = threadIdx.x & 15;
    float ls[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) ls[e] = ls1[sub * 8 + e];
    const int n_items = (int)(M * 16);
    for (int item = blockIdx.x * 256 + threadIdx.x; item < n_items; item += gridDim.x * 256) {
        const int64_t tok = item >> 4;
        const int node = node_of(item >> 4, Tn, mode);
        const float sc = sC[node][0], sh = sC[node][1];
        float a[8], b[8], c[8];
        load8(x_in + tok * 128 + sub * 8, a);
        load8(xn + tok * 128 + sub * 8, b);
        load8(y + tok * 128 + sub * 8, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float z = b[e] + c[e] * sc + sh;
            a[e] += ls[e] * (z != z ? z : fmaxf(z, 0.f));           // fmaxf drops a NaN; F.relu keeps it (a poisoned statistic must reach the output: graph.py:128-129)
        }
        store8(out + tok * 128 + sub * 8, a);
    }
}

// ------------------------------------------------------------------ backward, stage 1: through layer-scale and ReLU; BN-backward sums
template <typename T>
__global__ __launch_bounds__(256) void k_gcn_bwd1(const T* __restrict__ g, const T* __restrict__ xn, const T* __restrict__ y, const float* __restrict__ coef,
                                                  const float* __restrict__ ls1, T* __restrict__ rbuf, float* __restrict__ dls1,
                                                  double* __restrict__ bstats, int64_t M, int Tn, int mode, int nodes, float* __restrict__ dls_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem_b1[];
    float* sStat = reinterpret_cast<float*>(smem_b1);   // [16][2 nodes]: one private row per 16-lane group (see k_gcn_agg_spatial)
    __shared__ float sRed[16 * 128];
    for (int idx = threadIdx.x; idx < 16 * 2 * nodes; idx += 256) sStat[idx] = 0.f;
    __syncthreads();
    const int sub = threadIdx.x & 15, rl = threadIdx.x >> 4;
    float ls[8], dls[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ls[e] = ls1[sub * 8 + e]; dls[e] = 0.f; }
    // two items per pass, all six loads issued before the first use: at 512 workgroups (the block-end atomics are same-address) one item per pass
    // leaves only 3 x 16 bytes per lane in flight, 3.1 TB/s
    const int n_items = (int)(M * 16), stride = gridDim.x * 256;
    for (int item0 = blockIdx.x * 256 + threadIdx.x; item0 < n_items; item0 += 2 * stride) {
        const int item1 = item0 + stride;
        const bool has1 = item1 < n_items;
        const int tk[2] = {item0 >> 4, has1 ? item1 >> 4 : item0 >> 4};
        float gg[2][8], b[2][8], c[2][8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t tok = tk[u];
            load8(g + tok * 128 + sub * 8, gg[u]);
            load8(xn + tok * 128 + sub * 8, b[u]);
            load8(y + tok * 128 + sub * 8, c[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !has1) break;
            const int64_t tok = tk[u];
            const int node = node_of(tk[u], Tn, mode);
            const float sc = coef[node * COEF_LD], sh = coef[node * COEF_LD + 1], mean = coef[node * COEF_LD + 2], rstd = coef[node * COEF_LD + 3];
            float r[8];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float z = b[u][e] + c[u][e] * sc + sh;
                dls[e] += gg[u][e] * fmaxf(z, 0.f);
                r[e] = z > 0.f ? ls[e] * gg[u][e] : 0.f;
                s1 += r[e];
                s2 += r[e] * (c[u][e] - mean) * rstd;
            }
            store8(rbuf + tok * 128 + sub * 8, r);
            s1 = reduce16(s1);
            s2 = reduce16(s2);
            if (sub == 0) { sStat[rl * 2 * nodes + node * 2] += s1; sStat[rl * 2 * nodes + node * 2 + 1] += s2; }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sRed[rl * 128 + sub * 8 + e] = dls[e];
    __syncthreads();
    if (threadIdx.x < 128) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += sRed[k * 128 + threadIdx.x];
        if (dls_rows != nullptr) dls_rows[(int64_t)blockIdx.x * 128 + threadIdx.x] = s;      // one row per workgroup, added in a fixed order by k_col_finish
        else atomicAdd(dls1 + threadIdx.x, s);
    }
    for (int idx = threadIdx.x; idx < 2 * nodes; idx += 256) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sStat[k * 2 * nodes + idx];
        stat_add(stat_slot(bstats), idx, (double)t);
    }
}

// dy of one 8-channel chunk: BN backward with the finalised per-node means
// sC: per-node {scale, mean, rstd, c1, c2} in LDS (c1, c2 = the BatchNorm-backward means, derived per workgroup by bwd2_prologue)
constexpr int C2_LD = 5;
__device__ __forceinline__ void dy_math(const float (&r)[8], const float (&c)[8], const float* sC, int node, float (&dy)[8]) {
    const float sc = sC[node * C2_LD], mean = sC[node * C2_LD + 1], rstd = sC[node * C2_LD + 2];
    const float c1 = sC[node * C2_LD + 3], c2 = sC[node * C2_LD + 4];
#pragma unroll
    for (int e = 0; e < 8; ++e) dy[e] = sc * (r[e] - c1 - (c[e] - mean) * rstd * c2);
}
template <typename T>
__device__ __forceinline__ void dy_chunk(const T* rbuf, const T* y, const float* sC, int64_t tok, int node, int sub, float (&dy)[8]) {
    float r[8], c[8];
    load8(rbuf + tok * 128 + sub * 8, r);
    load8(y + tok * 128 + sub * 8, c);
    dy_math(r, c, sC, node, dy);
}

// what k_gcn_bwd_finalize did in a one-workgroup launch: every workgroup derives the node table itself; workgroup 0 accumulates d(bn weight / bias)
__device__ __forceinline__ void bwd2_prologue(float* sC, const float* coef, const double* bstats, float* d_w, float* d_b, int nodes, double count,
                                              int training) {
    if ((int)threadIdx.x < nodes) {
        const int n = threadIdx.x;
        sC[n * C2_LD + 0] = coef[n * COEF_LD];
        sC[n * C2_LD + 1] = coef[n * COEF_LD + 2];
        sC[n * C2_LD + 2] = coef[n * COEF_LD + 3];
        const double s0 = stat_sum(bstats, 2 * n), s1 = stat_sum(bstats, 2 * n + 1);
        sC[n * C2_LD + 3] = training ? (float)(s0 / count) : 0.f;      // evaluation-mode BatchNorm: mean / variance are constants, dy = scale * r
        sC[n * C2_LD + 4] = training ? (float)(s1 / count) : 0.f;
        if (blockIdx.x == 0) {
            d_b[n] += (float)s0;
            d_w[n] += (float)s1;
        }
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void k_gcn_bwd2_spatial(const T* __restrict__ rbuf, const T* __restrict__ y, const float* __restrict__ coefg,
                                                          T* __restrict__ duv, int64_t M, const double* __restrict__ bstats, float* __restrict__ d_w,
                                                          float* __restrict__ d_b, int nodes, double count, int training) {
    __shared__ float coef[KASF_MAX_NODES * C2_LD];
    bwd2_prologue(coef, coefg, bstats, d_w, d_b, nodes, count, training);
    const int sub = threadIdx.x & 15;
    const int n_items = (int)(M * 16);
    for (int item = blockIdx.x * 256 + threadIdx.x; item < n_items; item += gridDim.x * 256) {
        const int tk = item >> 4, fr = (tk / KASF_J) * KASF_J;
        const int64_t tok = tk, frame0 = fr;
        const int i = tk - fr;
        float dy[8], dv[8];
        dy_chunk(rbuf, y, coef, tok, i, sub, dy);
        store8(duv + tok * 256 + sub * 8, dy);                       // dU = dy
#pragma unroll
        for (int e = 0; e < 8; ++e) dv[e] = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {                                // A_hat is symmetric: dV_i = sum_nb coef * dy_nb  (the branch-free gather of k_gcn_agg_spatial measured +3 % here: five
            const int nb = c_skel.nb[i][e];                          //  dy_chunk evaluations in flight instead of one at a time; round 5)
            if (nb >= 0) {
                float t[8];
                dy_chunk(rbuf, y, coef, frame0 + nb, nb, sub, t);
                const float c = c_skel.coef[i][e];
#pragma unroll
                for (int k = 0; k < 8; ++k) dv[k] += c * t[k];
            }
        }
        store8(duv + tok * 256 + 128 + sub * 8, dv);
    }
}

template <typename T, int L>
__global__ __launch_bounds__(256) void k_gcn_bwd2_temporal(const T* __restrict__ rbuf, const T* __restrict__ y, const float* __restrict__ coefg,
                                                           const uint32_t* __restrict__ mask, T* __restrict__ duv, int Tn, const double* __restrict__ bstats,
                                                           float* __restrict__ d_w, float* __restrict__ d_b, int nodes, double count, int training) {
    __shared__ float coef[KASF_MAX_NODES * C2_LD];
    bwd2_prologue(coef, coefg, bstats, d_w, d_b, nodes, count, training);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sDy = reinterpret_cast<float*>(smem);        // [L][SX_LD]
    float* sDinv = sDy + L * SX_LD;
    uint32_t* sMask = reinterpret_cast<uint32_t*>(sDinv + L);
    const int G = blockIdx.x, b = G / KASF_J, j = G % KASF_J;
    auto tok = [&](int r) { return ((int64_t)b * Tn + r) * KASF_J + j; };
    for (int idx = threadIdx.x; idx < L * 16; idx += 256) {
        const int r = idx >> 4, sub = idx & 15;
        float dy[8];
        dy_chunk(rbuf, y, coef, tok(r), r, sub, dy);
        store8(duv + tok(r) * 256 + sub * 8, dy);
#pragma unroll
        for (int e = 0; e < 8; ++e) sDy[r * SX_LD + sub * 8 + e] = dy[e];
    }
    for (int r = threadIdx.x; r < L; r += 256) {
        int deg = 0;
#pragma unroll
        for (int e = 0; e < MASK_W; ++e) { const uint32_t w = mask[((int64_t)G * L + r) * MASK_W + e]; sMask[r * MASK_W + e] = w; deg += __popc(w); }
        sDinv[r] = 1.0f / sqrtf((float)deg);
    }
    __syncthreads();
    // The transposed aggregate needs, per column c, the rows r whose mask has bit c.  Testing all L rows per (column, chunk) item was the launch (81 x 81
    // bit tests with an LDS read each, 116 us at T = 81): transpose the bit matrix once per track with wave ballots (lane = row, one ballot per column and
    // 64-row half) and then visit set bits only, in ascending row order as before (same summation order: bit-identical results).
    uint32_t* sMaskT = sMask + L * MASK_W;              // [L][MASK_W]: bit r of column c's words
    {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int c = w; c < L; c += 4) {
#pragma unroll
            for (int h = 0; h < (L + 63) / 64; ++h) {
                const int r = 64 * h + lane;
                const bool bit = r < L && ((sMask[r * MASK_W + (c >> 5)] >> (c & 31)) & 1u);
                const unsigned long long bal = __ballot(bit);
                if (lane == 0) {
                    sMaskT[c * MASK_W + 2 * h] = (uint32_t)bal;
                    if (2 * h + 1 < MASK_W) sMaskT[c * MASK_W + 2 * h + 1] = (uint32_t)(bal >> 32);
                }
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < L * 16; idx += 256) {
        const int c = idx >> 4, sub = idx & 15;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        const float dc = sDinv[c];
#pragma unroll
        for (int wi = 0; wi < (L + 31) / 32; ++wi) {
            uint32_t bits = sMaskT[c * MASK_W + wi];
            while (bits) {
                const int r = wi * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                const float w = sDinv[r] * dc;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += w * sDy[r * SX_LD + sub * 8 + e];
            }
        }
        store8(duv + tok(c) * 256 + 128 + sub * 8, acc);
    }
}

// ------------------------------------------------------------------ temporal aggregate / backward for ANY number of frames (4 <= T <= 256)
// The instantiations above keep the whole T x T similarity matrix of a track in LDS, which stops fitting near T = 100.  Here S never leaves the
// registers: a wave owns 16-row blocks of the track, runs the same MFMA products in the same k order (S stays bitwise symmetric) against every
// 16-column tile -- lane (row li, group lg) ends up with its row's columns 16 tn + 4 lg + {0..3}, up to 64 values --, keeps the four largest as they
// come, merges them across the row's four lanes, and turns the kept values into mask words (the two tiles of a word OR-ed across the four lanes).
// No similarity tile in LDS, no barrier per row block; only the masks (T x MW words) and degrees of the track stay resident, and the LN(x) tile is then
// overwritten by the V rows for the aggregation.  (First version: S through LDS 16 rows at a time and one thread scanning each row: 1.46 ms per launch
// at T = 243, B = 32; 16 lanes per row + ballots: 0.35 ms.)
template <typename T>
__global__ __launch_bounds__(256) void k_gcn_agg_temporal_g(const T* __restrict__ uv, const T* __restrict__ xn, T* __restrict__ y,
                                                            uint32_t* __restrict__ mask, double* __restrict__ stats, int L, int MW, int kth, int n_tracks) {
    constexpr int EPC = Tile<T>::EPC, CPR = Tile<T>::CPR;
    const int LP = (L + 15) / 16 * 16, NTL = LP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* sX = reinterpret_cast<T*>(smem);                 // [LP][128] swizzled LN(x) rows, later [L][128] linear V rows
    float* sDinv = reinterpret_cast<float*>(sX + LP * 128);   // [L]
    float* sStat = sDinv + LP;                          // [L][2]
    uint32_t* sMask = reinterpret_cast<uint32_t*>(sStat + 2 * LP);   // [L][MW]
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4;
    for (int idx = threadIdx.x; idx < 2 * L; idx += 256) sStat[idx] = 0.f;
    for (int G = blockIdx.x; G < n_tracks; G += gridDim.x) {
        const int b = G / KASF_J, j = G % KASF_J;
        auto tok = [&](int r) { return ((int64_t)b * L + r) * KASF_J + j; };
        __syncthreads();
        for (int i0 = threadIdx.x; i0 < LP * CPR; i0 += 1024) {     // (four chunks' loads in flight per thread)
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = i0 + 256 * k, r = idx / CPR, ch = idx % CPR;
                v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (r < L) v[k] = *reinterpret_cast<const f32x4*>(xn + tok(r) * 128 + ch * EPC);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = i0 + 256 * k, r = idx / CPR, ch = idx % CPR;
                if (idx < LP * CPR) *reinterpret_cast<f32x4*>(sX + Tile<T>::chunk_off(r, ch)) = v[k];
            }
        }
        __syncthreads();
        for (int rb = w; rb < NTL; rb += 4) {
            const int r = rb * 16 + li;                 // this lane's row; it sees columns 16 tn + 4 lg + q
            f32x4 sv[16];
            float top[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int tn = 0; tn < 16; ++tn) {
                if (tn < NTL) {
                    f32x4 acc[1][1];
                    zero_acc(acc);
                    mma_k128<1, 1>(sX, tn * 16, sX, rb * 16, acc);
                    sv[tn] = acc[0][0];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float v = tn * 16 + 4 * lg + q < L ? acc[0][0][q] : -INFINITY;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {      // compare-exchange as max / min (S is finite)
                            const float hi = fmaxf(top[e], v);
                            v = fminf(top[e], v);
                            top[e] = hi;
                        }
                    }
                }
            }
#pragma unroll
            for (int m = 16; m <= 32; m <<= 1) {           // the row's other three lanes
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = __shfl_xor(top[e], m);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = o[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float hi = fmaxf(top[e], v);
                        v = fminf(top[e], v);
                        top[e] = hi;
                    }
                }
            }
            // k-th largest of the row (with multiplicity) -> adjacency bits and degree (graph.py:104-112: ties kept)
            const float thr = kth <= 1 ? top[0] : (kth == 2 ? top[1] : (kth == 3 ? top[2] : top[3]));
            int deg = 0;
#pragma unroll
            for (int wi = 0; wi < 8; ++wi) {
                if (wi < MW) {
                    uint32_t bits = 0u;
#pragma unroll
                    for (int half = 0; half < 2; ++half) {
                        const int tn = 2 * wi + half;
                        if (tn < NTL) {
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (tn * 16 + 4 * lg + q < L && sv[tn][q] >= thr) bits |= 1u << (half * 16 + 4 * lg + q);
                        }
                    }
                    bits |= (uint32_t)__shfl_xor((int)bits, 16);
                    bits |= (uint32_t)__shfl_xor((int)bits, 32);
                    deg += __popc(bits);
                    if (lg == 0 && r < L) {
                        sMask[r * MW + wi] = bits;
                        mask[((int64_t)G * L + r) * MW + wi] = bits;
                    }
                }
            }
            if (lg == 0 && r < L) sDinv[r] = 1.0f / sqrtf((float)deg);
        }
        __syncthreads();
        for (int i0 = threadIdx.x; i0 < L * CPR; i0 += 1024) {       // the similarity is done with LN(x): the tile now holds the V rows (linear)
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = i0 + 256 * k, r = idx / CPR, ch = idx % CPR;
                if (idx < L * CPR) v[k] = *reinterpret_cast<const f32x4*>(uv + tok(r) * 256 + 128 + ch * EPC);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = i0 + 256 * k, r = idx / CPR, ch = idx % CPR;
                if (idx < L * CPR) *reinterpret_cast<f32x4*>(sX + r * 128 + ch * EPC) = v[k];
            }
        }
        float un[8];
        if ((int)threadIdx.x < L * 16) load8(uv + tok(threadIdx.x >> 4) * 256 + (threadIdx.x & 15) * 8, un);
        __syncthreads();
        for (int idx = threadIdx.x; idx < L * 16; idx += 256) {
            const int r = idx >> 4, sub = idx & 15;
            float acc[8], u[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) u[e] = un[e];
            if (idx + 256 < L * 16) load8(uv + tok((idx + 256) >> 4) * 256 + sub * 8, un);     // U of the next item rides under this item's gather
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            const float dr = sDinv[r];
            for (int wi = 0; wi < MW; ++wi) {
                uint32_t bits = sMask[r * MW + wi];
                while (bits) {
                    const int c = wi * 32 + __builtin_ctz(bits);
                    bits &= bits - 1;
                    const float wgt = dr * sDinv[c];
                    float v[8];
                    load8(sX + c * 128 + sub * 8, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += wgt * v[e];
                }
            }
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { acc[e] += u[e]; const float q = to_f(from_f<T>(acc[e])); s1 += q; s2 += q * q; }
            store8(y + tok(r) * 128 + sub * 8, acc);
            s1 = reduce16(s1);
            s2 = reduce16(s2);
            if (sub == 0) { atomicAdd(&sStat[r * 2], s1); atomicAdd(&sStat[r * 2 + 1], s2); }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * L; idx += 256) stat_add(stat_slot(stats), idx, (double)sStat[idx]);
}

template <typename T>
__global__ __launch_bounds__(256) void k_gcn_bwd2_temporal_g(const T* __restrict__ rbuf, const T* __restrict__ y, const float* __restrict__ coefg,
                                                             const uint32_t* __restrict__ mask, T* __restrict__ duv, int L, int MW,
                                                             const double* __restrict__ bstats, float* __restrict__ d_w, float* __restrict__ d_b, double count,
                                                             int training) {
    __shared__ float coef[KASF_MAX_NODES * C2_LD];
    bwd2_prologue(coef, coefg, bstats, d_w, d_b, L, count, training);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int DY_LD = 128 + 16 / sizeof(T);         // dy rows in the storage type (bf16 mode: the rounded values dU stores; 64 KB at T = 243: two workgroups per CU)
    T* sDy = reinterpret_cast<T*>(smem);                // [L][DY_LD]
    float* sDinv = reinterpret_cast<float*>(sDy + L * DY_LD);
    uint32_t* sMask = reinterpret_cast<uint32_t*>(sDinv + L);
    const int G = blockIdx.x, b = G / KASF_J, j = G % KASF_J;
    auto tok = [&](int r) { return ((int64_t)b * L + r) * KASF_J + j; };
    // (four items' loads in flight per thread: with two workgroups per CU a load -> store chain per item pays the memory latency 15 times over at T = 243)
    for (int i0 = threadIdx.x; i0 < L * 16; i0 += 1024) {
        float rr[4][8], cc[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = i0 + 256 * k;
            if (idx < L * 16) {
                load8(rbuf + tok(idx >> 4) * 128 + (idx & 15) * 8, rr[k]);
                load8(y + tok(idx >> 4) * 128 + (idx & 15) * 8, cc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = i0 + 256 * k;
            if (idx < L * 16) {
                const int r = idx >> 4, sub = idx & 15;
                float dy[8];
                dy_math(rr[k], cc[k], coef, r, dy);
                store8(duv + tok(r) * 256 + sub * 8, dy);
                store8(sDy + r * DY_LD + sub * 8, dy);
            }
        }
    }
    for (int r = threadIdx.x; r < L; r += 256) {
        int deg = 0;
        for (int e = 0; e < MW; ++e) { const uint32_t wd = mask[((int64_t)G * L + r) * MW + e]; sMask[r * MW + e] = wd; deg += __popc(wd); }
        sDinv[r] = 1.0f / sqrtf((float)deg);
    }
    __syncthreads();
    // the bit matrix transposed once per track with wave ballots (lane = row), then set bits only, in ascending row order -- as k_gcn_bwd2_temporal does
    // (testing all L rows per (column, chunk) item was 0.7 ms per launch at T = 243, B = 32)
    uint32_t* sMaskT = sMask + L * MW;                  // [L][MW]: bit r of column c's words
    {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        for (int c = w; c < L; c += 4) {
            uint32_t wd[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {               // (the column's four reads are in flight together)
                const int r = 64 * h + lane;
                wd[h] = (2 * h < MW && r < L) ? sMask[r * MW + (c >> 5)] : 0u;
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                if (2 * h < MW) {
                    const unsigned long long bal = __ballot((wd[h] >> (c & 31)) & 1u);
                    if (lane == 0) {
                        sMaskT[c * MW + 2 * h] = (uint32_t)bal;
                        if (2 * h + 1 < MW) sMaskT[c * MW + 2 * h + 1] = (uint32_t)(bal >> 32);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < L * 16; idx += 256) {
        const int c = idx >> 4, sub = idx & 15;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        const float dc = sDinv[c];
        for (int wi = 0; wi < MW; ++wi) {
            uint32_t bits = sMaskT[c * MW + wi];
            while (bits) {
                const int r = wi * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                const float wgt = sDinv[r] * dc;
                float v[8];
                load8(sDy + r * DY_LD + sub * 8, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += wgt * v[e];
            }
        }
        store8(duv + tok(c) * 256 + 128 + sub * 8, acc);
    }
}

inline unsigned ew_grid(int64_t M) {
    int64_t blocks = (M * 16 + 255) / 256;
    return (unsigned)(blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks));
}
template <typename K> void set_smem(K k, size_t bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
template <typename T, int L> constexpr size_t agg_smem() {
    return (size_t)agg_lp<L>() * 128 * sizeof(T) + agg_region2<T, L>() + (L + 2 * L) * sizeof(float) + L * MASK_W * sizeof(uint32_t);
}
template <int L> constexpr size_t bwd2_smem() { return (L * SX_LD + L) * sizeof(float) + 2 * L * MASK_W * sizeof(uint32_t); }

template <typename T, int L>
void agg_temporal_TL(hipStream_t s, const void* uv, const void* xn, void* y, uint32_t* mask, double* stats, int B, int Tn, int kth) {
    const size_t sh = agg_smem<T, L>();
    set_smem(k_gcn_agg_temporal<T, L>, sh);
    // persistent workgroups, equal track counts, ONE round: never more workgroups than fit on the chip at once (LDS bound; T = 81: 2 per CU -- 726
    // workgroups of 3 tracks ran as a full round and a 42 % round, six track-times where five do)
    int per_cu = (int)(160 * 1024 / sh);
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    const int tracks = B * KASF_J, resident = 256 * per_cu, per = (tracks + resident - 1) / resident;
    hipLaunchKernelGGL((k_gcn_agg_temporal<T, L>), dim3((tracks + per - 1) / per), dim3(256), sh, s, (const T*)uv, (const T*)xn, (T*)y, mask,
                       stats, Tn, kth, tracks);
}
template <typename T, int L>
void bwd2_temporal_TL(hipStream_t s, const void* r, const void* y, const float* coef, const uint32_t* mask, void* duv, int B, int Tn, const double* bstats,
                      float* d_w, float* d_b, double count, int training) {
    set_smem(k_gcn_bwd2_temporal<T, L>, bwd2_smem<L>());
    hipLaunchKernelGGL((k_gcn_bwd2_temporal<T, L>), dim3(B * KASF_J), dim3(256), bwd2_smem<L>(), s, (const T*)r, (const T*)y, coef, mask, (T*)duv, Tn, bstats,
                       d_w, d_b, Tn, count, training);
}

template <typename T>
void agg_fwd_T(hipStream_t s, const void* uv, const void* xn, void* y, uint32_t* mask, double* stats, int B, int Tn, int mode, int kth) {
    const int64_t M = (int64_t)B * Tn * KASF_J;
    if (mode == 0) {
        unsigned grid = ew_grid(M);
        if (grid > 1024) grid = 1024;                    // every workgroup ends with 34 same-address fp64 atomics
        hipLaunchKernelGGL(k_gcn_agg_spatial<T>, dim3(grid), dim3(256), 0, s, (const T*)uv, (T*)y, stats, M);
    } else if (Tn == 27) agg_temporal_TL<T, 27>(s, uv, xn, y, mask, stats, B, Tn, kth);
#ifndef KASF_AGG81_G
    else if (Tn == 81) agg_temporal_TL<T, 81>(s, uv, xn, y, mask, stats, B, Tn, kth);
#endif
    else if (Tn == 9) agg_temporal_TL<T, 9>(s, uv, xn, y, mask, stats, B, Tn, kth);
    else {
        const int LP = (Tn + 15) / 16 * 16, MW = kasf_gcn_mask_words(Tn);
        const size_t sh = (size_t)LP * 128 * sizeof(T) + (size_t)(3 * LP) * sizeof(float) + (size_t)Tn * MW * sizeof(uint32_t);
        set_smem(k_gcn_agg_temporal_g<T>, sh);
        const int tracks = B * KASF_J, per = (tracks + 1023) / 1024;
        hipLaunchKernelGGL((k_gcn_agg_temporal_g<T>), dim3((tracks + per - 1) / per), dim3(256), sh, s, (const T*)uv, (const T*)xn, (T*)y, mask, stats, Tn, MW, kth,
                           tracks);
    }
}
template <typename T>
void bwd2_T(hipStream_t s, const void* r, const void* y, const float* coef, const uint32_t* mask, void* duv, int B, int Tn, int mode, const double* bstats,
            float* d_w, float* d_b, double count, int training) {
    const int64_t M = (int64_t)B * Tn * KASF_J;
    if (mode == 0) hipLaunchKernelGGL(k_gcn_bwd2_spatial<T>, dim3(ew_grid(M)), dim3(256), 0, s, (const T*)r, (const T*)y, coef, (T*)duv, M, bstats, d_w, d_b,
                                      KASF_J, count, training);
    else if (Tn == 27) bwd2_temporal_TL<T, 27>(s, r, y, coef, mask, duv, B, Tn, bstats, d_w, d_b, count, training);
    else if (Tn == 81) bwd2_temporal_TL<T, 81>(s, r, y, coef, mask, duv, B, Tn, bstats, d_w, d_b, count, training);
    else if (Tn == 9) bwd2_temporal_TL<T, 9>(s, r, y, coef, mask, duv, B, Tn, bstats, d_w, d_b, count, training);
    else {
        const int MW = kasf_gcn_mask_words(Tn);
        const size_t sh = (size_t)Tn * (128 + 16 / sizeof(T)) * sizeof(T) + (size_t)Tn * sizeof(float) + (size_t)2 * Tn * MW * sizeof(uint32_t);
        set_smem(k_gcn_bwd2_temporal_g<T>, sh);
        hipLaunchKernelGGL((k_gcn_bwd2_temporal_g<T>), dim3(B * KASF_J), dim3(256), sh, s, (const T*)r, (const T*)y, coef, mask, (T*)duv, Tn, MW, bstats, d_w,
                           d_b, count, training);
    }
}

}  // namespace

// the skeleton table lives in constant memory, of which every device has its own copy: once per device (one process may drive several)
void kasf_gcn_init() {
    static bool ready[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && ready[dev]) return;
    // graph.py:16-17 -- copied as data (bit-exact indices); degree = number of listed neighbours
    static const int adj[KASF_J][4] = {{1, 7, 4, -1}, {2, 0, -1, -1}, {3, 1, -1, -1}, {2, -1, -1, -1}, {5, 0, -1, -1}, {6, 4, -1, -1},
                                       {5, -1, -1, -1}, {0, 8, -1, -1}, {7, 9, 11, 14}, {8, 10, -1, -1}, {9, -1, -1, -1}, {12, 8, -1, -1},
                                       {13, 11, -1, -1}, {12, -1, -1, -1}, {15, 8, -1, -1}, {16, 14, -1, -1}, {15, -1, -1, -1}};
    SkelTable t;
    int deg[KASF_J];
    for (int i = 0; i < KASF_J; ++i) { deg[i] = 0; for (int e = 0; e < 4; ++e) deg[i] += adj[i][e] >= 0; }
    for (int i = 0; i < KASF_J; ++i)
        for (int e = 0; e < 4; ++e) {
            t.nb[i][e] = adj[i][e];
            t.coef[i][e] = adj[i][e] >= 0 ? (1.0f / sqrtf((float)deg[i])) * (1.0f / sqrtf((float)deg[adj[i][e]])) : 0.f;
        }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_skel), &t, sizeof(t));
    if (dev >= 0 && dev < 64) ready[dev] = true;
}

void kasf_launch_gcn_agg_fwd(int dt, hipStream_t s, const void* uv, const void* xn, void* y, uint32_t* mask, double* stats, int B, int T, int mode, int kth) {
    kasf_gcn_init();
    if (dt == KASF_F32) agg_fwd_T<float>(s, uv, xn, y, mask, stats, B, T, mode, kth);
    else agg_fwd_T<bf16>(s, uv, xn, y, mask, stats, B, T, mode, kth);
}
void kasf_launch_gcn_apply(int dt, hipStream_t s, const void* x_in, const void* xn, const void* y, const double* stats, const float* bn_w, const float* bn_b,
                           float* run_mean, float* run_var, float* coef, const float* ls1, void* out, int B, int T, int mode, double count, int training,
                           float momentum) {
    const int64_t M = (int64_t)B * T * KASF_J;
    const int nodes = mode == 0 ? KASF_J : T;
    if (dt == KASF_F32) hipLaunchKernelGGL(k_gcn_apply<float>, dim3(ew_grid(M)), dim3(256), 0, s, (const float*)x_in, (const float*)xn, (const float*)y, stats, bn_w, bn_b, run_mean, run_var, coef, ls1, (float*)out, M, T, mode, nodes, count, training, momentum);
    else hipLaunchKernelGGL(k_gcn_apply<bf16>, dim3(ew_grid(M)), dim3(256), 0, s, (const bf16*)x_in, (const bf16*)xn, (const bf16*)y, stats, bn_w, bn_b, run_mean, run_var, coef, ls1, (bf16*)out, M, T, mode, nodes, count, training, momentum);
}
int kasf_gcn_bwd1_rows(int64_t M) {
    const unsigned grid = ew_grid(M);
    return (int)(grid > 512 ? 512 : grid);               // block-end atomics on the BN sums are same-address
}
void kasf_launch_gcn_bwd1(int dt, hipStream_t s, const void* g, const void* xn, const void* y, const float* coef, const float* ls1, void* r,
                          float* dls1, double* bstats, int B, int T, int mode, KasfColSink* sink) {
    const int64_t M = (int64_t)B * T * KASF_J;
    const int nodes = mode == 0 ? KASF_J : T;
    const unsigned grid = (unsigned)kasf_gcn_bwd1_rows(M);
    const size_t sh = (size_t)16 * 2 * nodes * sizeof(float);
    float* rows = sink != nullptr ? sink->take((int)grid, 128) : nullptr;
    if (dt == KASF_F32) hipLaunchKernelGGL(k_gcn_bwd1<float>, dim3(grid), dim3(256), sh, s, (const float*)g, (const float*)xn, (const float*)y, coef, ls1, (float*)r, dls1, bstats, M, T, mode, nodes, rows);
    else hipLaunchKernelGGL(k_gcn_bwd1<bf16>, dim3(grid), dim3(256), sh, s, (const bf16*)g, (const bf16*)xn, (const bf16*)y, coef, ls1, (bf16*)r, dls1, bstats, M, T, mode, nodes, rows);
    if (rows != nullptr) sink->add(rows, 128, (int)grid, 128, dls1);
}
void kasf_launch_gcn_bwd2(int dt, hipStream_t s, const void* r, const void* y, const float* coef, const uint32_t* mask, void* duv, int B, int T,
                          int mode, const double* bstats, float* d_bn_w, float* d_bn_b, double count, int training) {
    kasf_gcn_init();
    if (dt == KASF_F32) bwd2_T<float>(s, r, y, coef, mask, duv, B, T, mode, bstats, d_bn_w, d_bn_b, count, training);
    else bwd2_T<bf16>(s, r, y, coef, mask, duv, B, T, mode, bstats, d_bn_w, d_bn_b, count, training);
}
