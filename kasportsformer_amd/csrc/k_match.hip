// The keypoint tracks that C calibrated cameras' trackers emit -> which row of which camera is the same player (kasf.h, kasf_match_pair_costs /
// kasf_match_groups).  match_sample is the one statement of the pair rule's arithmetic: every line is the rounded fp64 operation(s) kasf.h names, by its
// parentheses, then left to right (-ffp-contract=off, a correctly rounded divide and square root); the camera model is camera_model.h's, "usable" is
// one_euro.h's, the assignment is assignment.h's.
//
// PAIR COSTS.  Two launches.  k_match_pairs: a workgroup of 256 threads owns one camera pair a < b, one block of PB = min(P, 256 / P) rows of camera a, and
// one tile of MATCH_TILE = 256 frames; a thread owns one (row of a, row of b) pair of the block, up to 256 of them, with the pair's three sums (num and den
// in fp64, the count) in registers.  The tile is a run of 256 * J consecutive samples [x, y, score] of every row, walked in chunks of MATCH_CHUNK = 16
// samples: the PB + P rows' records of a chunk are fetched into registers (the next chunk's fetch is issued before this chunk's pair walk, which hides it),
// undistorted ONCE, and kept in LDS as the ray direction R^T (x, y, 1) -- three fp64 planes [16][PB + P], consecutive rows of b on consecutive addresses, the
// row of a a broadcast -- and a score plane (NaN: not usable).  No ray ever reaches global memory.  A row with no usable keypoint in the chunk is flagged (a
// ballot over the 16 lanes that staged it) and its pairs skip the chunk: tracks overlap only partly in time.  Camera b's rows are undistorted once per block
// of a's rows: at P = 64 that is 68 undistortions for 256 pair samples, at P = 22 33 for 242.  LDS: 232 + 452 * (PB + P) bytes, 30.2 KiB at P = 64 (DESIGN.md,
// "matching").  The tile's partial sums go to the workspace [tile][camera pair][P][P]; k_match_finish adds them in ascending tile order, one thread per output
// element -- cost[b][a][q][p] repeats the additions of cost[a][b][p][q] and so has its bits --, and writes +inf and 0 into the diagonal blocks.  No atomics;
// the order of every sum is fixed by the sample index alone, not by the grid, the block of rows or the other cameras.
//
// GROUPS.  k_match_groups: one launch, one wave64 workgroup, cameras in ascending order; lane = group while groups are handled, lane = row while rows are.
// The cost matrix [row][group] sits in LDS for assign_wave64.
#include "kernels.h"
#include "camera_model.h"
#include "one_euro.h"
#include "assignment.h"

#ifndef KASF_DYNAMIC_LDS
#define KASF_DYNAMIC_LDS(name) extern __shared__ __attribute__((aligned(16))) float name[]
#endif

namespace {

constexpr int MATCH_TILE = 256;                                 // frames per tile of the summation order
constexpr int MATCH_CHUNK = 16;                                 // samples staged at a time
constexpr int MATCH_THREADS = 256;
constexpr int MATCH_ROUNDS = 5;                                 // (PB + P) * MATCH_CHUNK <= 68 * 16 = 1088 <= 5 * 256 items
constexpr double kMatchHuge = 1.7976931348623157e308;           // the largest finite double: fabs(v) <= kMatchHuge is false for a NaN and for an infinity
constexpr double kMatchParallel = 1e-10;                        // the parallel test of kasf.h: det > kMatchParallel * (aa * bb)
constexpr double kMatchBig = 1e9;                               // BIG of kasf.h: the cost of a row to a group with no comparable member

__device__ inline float match_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }
__device__ inline float match_inf() { return __builtin_bit_cast(float, 0x7f800000u); }
__device__ inline unsigned long long match_below(int lane) { return (1ull << lane) - 1ull; }

__host__ __device__ inline int match_block_rows(int P) {
    const int pb = MATCH_THREADS / P;
    return pb < 1 ? 1 : (pb > P ? P : pb);
}

// One sample of one pair: the rays (a, from oa, f = fa) and (b, from ob, fb).  Returns whether it is comparable, and then e.
__device__ inline bool match_sample(double ax, double ay, double az, double bx, double by, double bz, const double* oa, const double* ob, double fa, double fb,
                                    double& e) {
    const double wx = oa[0] - ob[0], wy = oa[1] - ob[1], wz = oa[2] - ob[2];
    const double aa = ax * ax + ay * ay + az * az;
    const double bb = bx * bx + by * by + bz * bz;
    const double ab = ax * bx + ay * by + az * bz;
    const double da = ax * wx + ay * wy + az * wz;
    const double db = bx * wx + by * wy + bz * wz;
    const double det = aa * bb - ab * ab;
    if (!(det > kMatchParallel * (aa * bb))) return false;
    const double s = (ab * db - bb * da) / det;
    const double t = (aa * db - ab * da) / det;
    if (!(s > 0.0) || !(t > 0.0) || !(s <= kMatchHuge) || !(t <= kMatchHuge)) return false;
    const double gx = (oa[0] + s * ax) - (ob[0] + t * bx);
    const double gy = (oa[1] + s * ay) - (ob[1] + t * by);
    const double gz = (oa[2] + s * az) - (ob[2] + t * bz);
    const double g = sqrt(gx * gx + gy * gy + gz * gz);
    e = 0.5 * g * (fa / s + fb / t);
    return fabs(e) <= kMatchHuge;
}

__global__ __launch_bounds__(MATCH_THREADS) void k_match_pairs(const float* __restrict__ keypoints, int C, int P, int64_t N, int J,
                                                               const float* __restrict__ cameras, KasfMatch p, double* __restrict__ ws_num,
                                                               double* __restrict__ ws_den, int* __restrict__ ws_cnt) {
    KASF_DYNAMIC_LDS(sm);
    const int PB = match_block_rows(P), R = PB + P, nblk = (P + PB - 1) / PB;
    double* s_org = reinterpret_cast<double*>(sm);              // [2][4]: the centre o = -R^T t and f of camera a, of camera b
    double* s_d = s_org + 8;                                    // [3][MATCH_CHUNK][R]: the ray directions
    float* s_w = reinterpret_cast<float*>(s_d + 3 * MATCH_CHUNK * R);       // [MATCH_CHUNK][R]: the score, NaN where the sample is not usable
    float* s_cam = s_w + MATCH_CHUNK * R;                       // [2][21]
    int* s_live = reinterpret_cast<int*>(s_cam + 2 * kCamFloats);           // [R]: the row has a usable sample in this chunk
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int cp = (int)blockIdx.y / nblk, blk = (int)blockIdx.y % nblk;
    int a = 0, rem = cp;
    while (rem >= C - 1 - a) {
        rem -= C - 1 - a;
        ++a;
    }
    const int b = a + 1 + rem;
    const int64_t n0 = tile * MATCH_TILE;
    const int nf = (int)(N - n0 < MATCH_TILE ? N - n0 : MATCH_TILE);
    const int L = nf * J, chunks = (L + MATCH_CHUNK - 1) / MATCH_CHUNK;
    const int p0 = blk * PB, PBe = P - p0 < PB ? P - p0 : PB;
    const int items = R * MATCH_CHUNK, rounds = (items + MATCH_THREADS - 1) / MATCH_THREADS;

    if (tid < 2 * kCamFloats) s_cam[tid] = cameras[(tid < kCamFloats ? a : b) * kCamFloats + tid % kCamFloats];
    __syncthreads();
    if (tid < 2) {
        const float* cam = s_cam + tid * kCamFloats;
        const double t0 = (double)cam[kCamT], t1 = (double)cam[kCamT + 1], t2 = (double)cam[kCamT + 2];
        for (int k = 0; k < 3; ++k)
            s_org[tid * 4 + k] = 0.0 - ((double)cam[kCamR + k] * t0 + (double)cam[kCamR + 3 + k] * t1 + (double)cam[kCamR + 6 + k] * t2);
        s_org[tid * 4 + 3] = 0.5 * ((double)cam[kCamFx] + (double)cam[kCamFy]);
    }
    const bool cam_ok_a = camera_finite(s_cam, kCamFloats), cam_ok_b = camera_finite(s_cam + kCamFloats, kCamFloats);
    __syncthreads();

    float kx[MATCH_ROUNDS], ky[MATCH_ROUNDS], ks[MATCH_ROUNDS];
    // the records of chunk ch -> registers; a sample past the tile's end or of a row past P comes as a NaN score
    auto fetch = [&](int ch) {
#pragma unroll
        for (int k = 0; k < MATCH_ROUNDS; ++k) {
            kx[k] = 0.0f, ky[k] = 0.0f, ks[k] = match_nan();
            const int item = k * MATCH_THREADS + tid;
            if (k < rounds && item < items) {
                const int r = item / MATCH_CHUNK, s = ch * MATCH_CHUNK + item % MATCH_CHUNK;
                const bool of_a = r < PB;
                if (s < L && (!of_a || r < PBe)) {
                    const int64_t row = (int64_t)(of_a ? a : b) * P + (of_a ? p0 + r : r - PB);
                    const float* src = keypoints + ((row * N + n0) * J + s) * 3;
                    kx[k] = src[0], ky[k] = src[1], ks[k] = src[2];
                }
            }
        }
    };

    double num = 0.0, den = 0.0;
    int cnt = 0;
    const bool owner = tid < PBe * P;
    const int ra = owner ? tid / P : 0, rb = owner ? PB + (tid - ra * P) : 0;
    const double fa = s_org[3], fb = s_org[7];
    const double cap = (double)p.cap;
    fetch(0);
    for (int ch = 0; ch < chunks; ++ch) {
#pragma unroll
        for (int k = 0; k < MATCH_ROUNDS; ++k) {
            if (k < rounds) {                                   // block-uniform: the ballot below is reached by every lane
                const int item = k * MATCH_THREADS + tid;
                const bool in = item < items;
                const int r = in ? item / MATCH_CHUNK : 0, i = item % MATCH_CHUNK;
                const float* cam = s_cam + (r < PB ? 0 : kCamFloats);
                const float k3[3] = {kx[k], ky[k], ks[k]};
                const bool ok = in && joint_usable<2>(k3, true, p.min_score) && (r < PB ? cam_ok_a : cam_ok_b);
                if (ok) {
                    double x, y;
                    camera_undistort(cam, k3[0], k3[1], p.undistort_iterations, x, y);
                    for (int c = 0; c < 3; ++c)
                        s_d[(c * MATCH_CHUNK + i) * R + r] = (double)cam[kCamR + c] * x + (double)cam[kCamR + 3 + c] * y + (double)cam[kCamR + 6 + c];
                }
                if (in) s_w[i * R + r] = ok ? k3[2] : match_nan();
                const unsigned long long usable = __ballot(ok);
                if (in && i == 0) s_live[r] = ((usable >> (tid & 48)) & 0xffffull) != 0ull;        // the row's 16 samples are 16 consecutive lanes
            }
        }
        __syncthreads();
        if (ch + 1 < chunks) fetch(ch + 1);
        if (owner && s_live[ra] && s_live[rb]) {
            for (int i = 0; i < MATCH_CHUNK; ++i) {
                const float wa = s_w[i * R + ra], wb = s_w[i * R + rb];
                if (!(wa == wa) || !(wb == wb)) continue;
                double e;
                if (!match_sample(s_d[i * R + ra], s_d[(MATCH_CHUNK + i) * R + ra], s_d[(2 * MATCH_CHUNK + i) * R + ra], s_d[i * R + rb],
                                  s_d[(MATCH_CHUNK + i) * R + rb], s_d[(2 * MATCH_CHUNK + i) * R + rb], s_org, s_org + 4, fa, fb, e))
                    continue;
                const double w = p.weighted ? (double)wa * (double)wb : 1.0;
                num = num + w * (e < cap ? e : cap);
                den = den + w;
                cnt += 1;
            }
        }
        __syncthreads();                                        // the next chunk overwrites the planes
    }
    if (owner) {
        const int64_t at = (tile * (C * (C - 1) / 2) + cp) * ((int64_t)P * P) + (int64_t)(p0 + ra) * P + (rb - PB);
        ws_num[at] = num;
        ws_den[at] = den;
        ws_cnt[at] = cnt;
    }
}

// one thread per element of cost / samples [C][C][P][P]
__global__ __launch_bounds__(MATCH_THREADS) void k_match_finish(const double* __restrict__ ws_num, const double* __restrict__ ws_den,
                                                                const int* __restrict__ ws_cnt, int C, int P, int64_t tiles, int min_samples,
                                                                float* __restrict__ cost, int* __restrict__ samples) {
    const int64_t PP = (int64_t)P * P, total = (int64_t)C * C * PP, at = (int64_t)blockIdx.x * MATCH_THREADS + threadIdx.x;
    if (at >= total) return;
    const int q = (int)(at % P), pr = (int)(at / P % P), b = (int)(at / PP % C), a = (int)(at / PP / C);
    if (a == b) {
        cost[at] = match_inf();
        samples[at] = 0;
        return;
    }
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const int64_t cp = (int64_t)lo * C - (int64_t)lo * (lo + 1) / 2 + (hi - lo - 1), pairs = (int64_t)(C * (C - 1) / 2) * PP;
    const int64_t src = cp * PP + (a < b ? (int64_t)pr * P + q : (int64_t)q * P + pr);
    double num = 0.0, den = 0.0;
    int cnt = 0;
    for (int64_t t = 0; t < tiles; ++t) {
        num = num + ws_num[t * pairs + src];
        den = den + ws_den[t * pairs + src];
        cnt += ws_cnt[t * pairs + src];
    }
    cost[at] = cnt >= min_samples ? (float)(num / den) : match_inf();
    samples[at] = cnt;
}

struct MatchGroupArgs {
    const float* cost;
    const int* samples;
    int *group, *members, *views;
    float* group_cost;
    int *count, *dropped;
    int C, P, G;
    float max_cost;
};

__global__ __launch_bounds__(64) void k_match_groups(const MatchGroupArgs A) {
    __shared__ double M[64 * ASSIGN_LD];                        // [row][group]
    __shared__ double got_cost[64];                             // [group]: the cost of the row it accepted from this camera
    __shared__ int mem[64 * 16];                                // [group][camera]: the member row, -1 for none
    __shared__ int rowlist[64], rowgrp[64], got[64];            // the non-empty rows, ascending | [row]: its group | [group]: it accepted a row of this camera
    const int lane = threadIdx.x, C = A.C, P = A.P, G = A.G;
    const int64_t PP = (int64_t)P * P;
    for (int i = lane; i < 64 * 16; i += 64) mem[i] = -1;
    int count = 0, dropped = 0;                                 // wave-uniform
    int views = 0, accepted = 0;                                // lane = group
    double cost_sum = 0.0;
    __syncthreads();
    for (int c = 0; c < C; ++c) {
        // ---- the non-empty rows of camera c: any sample against any row of any other camera ----
        bool full = false;
        if (lane < P)
            for (int m = 0; m < C; ++m) {
                if (m == c) continue;
                const int* s = A.samples + ((int64_t)c * C + m) * PP + (int64_t)lane * P;
                for (int r = 0; r < P; ++r) full = full || s[r] > 0;
            }
        const unsigned long long fm = __ballot(full);
        const int nr = __popcll(fm);
        if (full) rowlist[__popcll(fm & match_below(lane))] = lane;
        rowgrp[lane] = -1;
        got[lane] = 0;
        __syncthreads();
        const int row = lane < nr ? rowlist[lane] : -1;        // lane = position in the list of non-empty rows from here on
        int grp = -1;
        double grp_cost = 0.0;
        if (count > 0 && nr > 0) {                             // wave-uniform
            if (lane < count)                                  // lane = group: its column of the matrix
                for (int k = 0; k < nr; ++k) {
                    const int q = rowlist[k];
                    double num = 0.0, den = 0.0;
                    for (int m = 0; m < c; ++m) {
                        const int r = mem[lane * 16 + m];
                        if (r < 0) continue;
                        const int64_t at = ((int64_t)m * C + c) * PP + (int64_t)r * P + q;
                        const float cc = A.cost[at];
                        const int sm = A.samples[at];
                        if (fabsf(cc) <= 3.4028235e38f && sm > 0) {
                            num = num + (double)sm * (double)cc;
                            den = den + (double)sm;
                        }
                    }
                    M[k * ASSIGN_LD + lane] = den > 0.0 ? num / den : kMatchBig;
                }
            __syncthreads();
            int row_of_group;
            assign_wave64(M, nr, count, grp, row_of_group);
            if (grp >= 0) {
                grp_cost = M[lane * ASSIGN_LD + grp];
                if (grp_cost >= kMatchBig || grp_cost > (double)A.max_cost) grp = -1;
            }
        }
        if (grp >= 0) {
            got[grp] = 1;
            got_cost[grp] = grp_cost;
            mem[grp * 16 + c] = row;
        }
        // ---- rows without a group open new ones, in ascending row order, while there is room ----
        const bool loose = lane < nr && grp < 0;
        const unsigned long long lm = __ballot(loose);
        const int want = __popcll(lm), room = G - count, born = want < room ? want : room;
        if (loose && __popcll(lm & match_below(lane)) < born) {
            grp = count + __popcll(lm & match_below(lane));
            mem[grp * 16 + c] = row;
        }
        dropped += want - born;
        if (grp >= 0) rowgrp[row] = grp;
        __syncthreads();
        if (got[lane]) {                                       // lane = group
            views += 1;
            accepted += 1;
            cost_sum = cost_sum + got_cost[lane];
        }
        if (lane >= count && lane < count + born) views = 1;
        count += born;
        if (lane < P) A.group[c * P + lane] = rowgrp[lane];
        __syncthreads();
    }
    if (lane < G) {
        A.views[lane] = views;
        A.group_cost[lane] = accepted > 0 ? (float)(cost_sum / (double)accepted) : match_nan();
        for (int c = 0; c < C; ++c) A.members[lane * C + c] = mem[lane * 16 + c];
    }
    if (lane == 0) {
        *A.count = count;
        *A.dropped = dropped;
    }
}

}  // namespace

static int64_t match_tiles(int64_t N) { return (N + MATCH_TILE - 1) / MATCH_TILE; }

// the partial sums of every tile: num and den [tiles][C (C - 1) / 2][P][P] fp64, then the counts int32
int64_t kasf_match_workspace(int C, int P, int64_t N) { return match_tiles(N) * (C * (C - 1) / 2) * ((int64_t)P * P) * 20; }

// the LDS a pair-cost workgroup asks for: the two centres, three fp64 planes and a score plane [MATCH_CHUNK][PB + P], the two camera rows, the row flags
static size_t match_lds_bytes(int P) {
    const size_t R = (size_t)match_block_rows(P) + P;
    return 64 + R * MATCH_CHUNK * 28 + 2 * kCamFloats * 4 + R * 4;
}

// the arguments as the entry point checked them
void kasf_launch_match_pair_costs(hipStream_t s, const float* keypoints, int C, int P, int64_t N, int J, const float* cameras, const KasfMatch& p, float* cost,
                                  int* samples, void* workspace) {
    if (N <= 0) return;
    const int64_t tiles = match_tiles(N), slots = tiles * (C * (C - 1) / 2) * ((int64_t)P * P);
    double* ws_num = (double*)workspace;
    double* ws_den = ws_num + slots;
    int* ws_cnt = (int*)(ws_den + slots);
    const int PB = match_block_rows(P), nblk = (P + PB - 1) / PB;
    hipLaunchKernelGGL(k_match_pairs, dim3((unsigned)tiles, (unsigned)(C * (C - 1) / 2 * nblk)), dim3(MATCH_THREADS), match_lds_bytes(P), s, keypoints, C, P, N,
                       J, cameras, p, ws_num, ws_den, ws_cnt);
    const int64_t total = (int64_t)C * C * P * P;
    hipLaunchKernelGGL(k_match_finish, dim3((unsigned)((total + MATCH_THREADS - 1) / MATCH_THREADS)), dim3(MATCH_THREADS), 0, s, ws_num, ws_den, ws_cnt, C, P,
                       tiles, p.min_samples, cost, samples);
}

void kasf_launch_match_groups(hipStream_t s, const float* cost, const int* samples, int C, int P, float max_cost, int G, int* group, int* members, int* views,
                              float* group_cost, int* count, int* dropped) {
    MatchGroupArgs a;
    a.cost = cost; a.samples = samples; a.group = group; a.members = members; a.views = views; a.group_cost = group_cost; a.count = count; a.dropped = dropped;
    a.C = C; a.P = P; a.G = G; a.max_cost = max_cost;
    hipLaunchKernelGGL(k_match_groups, dim3(1), dim3(64), 0, s, a);
}
