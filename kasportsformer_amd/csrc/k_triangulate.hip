// Keypoints of one player seen by several calibrated cameras -> 3-D joints in the world frame (kasf.h, kasf_keypoints_triangulate), and the lens undistortion
// on its own (kasf_keypoints_undistort).  Per point -- one joint of one frame -- the C views' undistorted rays give a 3 x 3 weighted least-squares problem,
// Hartley and Zisserman's iteratively re-weighted linear triangulation with the placement's Cauchy weight.  tri_point is the one statement of the rule's
// arithmetic: every line is the rounded fp64 operation(s) kasf.h names, by its parentheses, then left to right (-ffp-contract=off, a correctly rounded divide
// and square root); the camera model is camera_model.h's, "usable" is one_euro.h's; results are rounded to fp32 once, at the store.
//
// One launch, one lane per point: a frame's 17 joints are 17 lanes, so one 18,000-frame track is 306,000 lanes where the placement's lane per frame has 18,000.
// 12 C + 18 B per point plus 4 C with the per-view residuals; the time is the lanes' chains of dependent fp64 divides, not the bytes (DESIGN.md,
// "triangulation").  A workgroup of two wavefronts owns TRI_TILE = 128 consecutive points.  View by view it stages the tile's 128 records [x, y, score] in LDS
// -- one float4 per lane on consecutive addresses where the view's tile is 16-byte aligned, one fp32 per lane otherwise and in the last, partial tile; the next
// view's load is issued before this view's undistortion, which hides it -- and lane i takes record i at LDS stride 3 words, an odd number of banks, undistorts
// it once and keeps the result as two fp64 planes and a score plane [C][128] in LDS (8- and 4-byte lane stride: no two lanes of an access share a bank).  The
// suggested in-place fp32 record would round x and y once more than the rule allows, so the planes are fp64: 20 B per view and point, which is why the tile is
// 128 and not 256 -- at C = 16 that is 42.8 KiB, three workgroups per CU and under the 64 KiB a launch gets without asking; 256 points would need 84 KiB.
// A pass of the fit then walks the views out of LDS (nothing is indexed in registers: no scratch) with its nine sums in fp64 registers.  A static rig's cameras
// sit in LDS; per-frame cameras are read through the cache, where a frame's 17 lanes share a row.  The points leave through the staging tile as whole rows
// (float4 where `points` is 16-byte aligned); residual, used, state and the per-view residuals are one element per lane on consecutive addresses, which a
// wavefront already stores as whole lines.  No atomics, no transcendental, every output element is written by one lane: the same bits from run to run, and a
// point's result depends on its own records and cameras alone, not on its neighbours, the grid or its place in the batch.
#include "kernels.h"
#include "camera_model.h"
#include "one_euro.h"

#ifndef KASF_DYNAMIC_LDS
#define KASF_DYNAMIC_LDS(name) extern __shared__ __attribute__((aligned(16))) float name[]
#endif

namespace {

constexpr int TRI_TILE = 128;                                   // points per workgroup pass = threads per workgroup
constexpr int TRI_TILE_FLOATS = TRI_TILE * 3;                   // 384: a multiple of 4, so every full tile starts 16-byte aligned when its view does
constexpr int UND_TILE = 256, UND_TILE_FLOATS = UND_TILE * 3;   // the undistortion alone: 3 KiB of static LDS
constexpr double kTriHuge = 1.7976931348623157e308;             // the largest finite double: fabs(v) <= kTriHuge is false for a NaN and for an infinity
constexpr double kTriPivot = 1e-9;                              // the pivot test of kasf.h: d > kTriPivot * trace(A)

__device__ inline float tri_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }
__device__ inline bool tri_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// 3 * count floats at src -> registers -> an LDS tile of TILE points.  vec: one float4 per lane (a full tile at a 16-byte aligned address), else one float per
// lane and round.  Two steps, so that a load can be in flight while the lanes compute.
template <int TILE>
__device__ inline void tile_fetch(const float* __restrict__ src, int count, bool vec, float (&r)[4]) {
    const int i = threadIdx.x;
    if (vec) {
        if (i < TILE * 3 / 4) {
            const float4 q = reinterpret_cast<const float4*>(src)[i];
            r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (i + k * TILE < count * 3) r[k] = src[i + k * TILE];
    }
}
template <int TILE>
__device__ inline void tile_stash(float* tile, int count, bool vec, const float (&r)[4]) {
    const int i = threadIdx.x;
    if (vec) {
        if (i < TILE * 3 / 4) reinterpret_cast<float4*>(tile)[i] = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (i + k * TILE < count * 3) tile[i + k * TILE] = r[k];
    }
}
// an LDS tile -> 3 * count floats at dst
template <int TILE>
__device__ inline void tile_store(const float* tile, int count, float* __restrict__ dst) {
    const int i = threadIdx.x;
    if (count == TILE && tri_aligned16(dst)) {
        if (i < TILE * 3 / 4) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(tile)[i];
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (i + k * TILE < count * 3) dst[i + k * TILE] = tile[i + k * TILE];
    }
}

// the nine sums of one pass: A = sum w a a^T (its six distinct entries) and b = sum w a r
struct TriSums {
    double a00, a01, a02, a11, a12, a22, b0, b1, b2;
};
__device__ inline void tri_row(TriSums& s, double w, double a0, double a1, double a2, double r) {
    s.a00 = s.a00 + w * (a0 * a0);
    s.a01 = s.a01 + w * (a0 * a1);
    s.a02 = s.a02 + w * (a0 * a2);
    s.a11 = s.a11 + w * (a1 * a1);
    s.a12 = s.a12 + w * (a1 * a2);
    s.a22 = s.a22 + w * (a2 * a2);
    s.b0 = s.b0 + w * (a0 * r);
    s.b1 = s.b1 + w * (a1 * r);
    s.b2 = s.b2 + w * (a2 * r);
}

// One point, steps 2 .. 4 of the rule.  sx, sy, sw: its undistorted x, y (fp64) and score (NaN: the view is not usable) of view v at index v * TRI_TILE; cam0:
// the camera row of view 0 for this point, view v's row cam_step floats further.  Leaves sqrt(rho) of every usable view in sx.  Returns the state.
__device__ inline int tri_point(double* sx, const double* sy, const float* sw, const float* cam0, int64_t cam_step, int C, int n_used, const KasfTriangulate& p,
                                double (&X)[3], double& res) {
    const double d2 = (double)p.delta * (double)p.delta;
    double X0 = 0.0, X1 = 0.0, X2 = 0.0, num = 0.0, den = 0.0;
    bool flat = false, behind = false;                          // a pivot failed or an X was not finite | a usable view had !(Z > 0)
    for (int pass = 0; pass <= p.iterations + 1; ++pass) {
        const bool last = pass == p.iterations + 1;
        TriSums s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int v = 0; v < C; ++v) {
            const float score = sw[v * TRI_TILE];
            if (!(score == score)) continue;                    // not usable
            const float* cam = cam0 + v * cam_step;
            const double x = sx[v * TRI_TILE], y = sy[v * TRI_TILE];
            const double fx = (double)cam[kCamFx], fy = (double)cam[kCamFy];
            const double r00 = (double)cam[kCamR], r01 = (double)cam[kCamR + 1], r02 = (double)cam[kCamR + 2];
            const double r10 = (double)cam[kCamR + 3], r11 = (double)cam[kCamR + 4], r12 = (double)cam[kCamR + 5];
            const double r20 = (double)cam[kCamR + 6], r21 = (double)cam[kCamR + 7], r22 = (double)cam[kCamR + 8];
            const double t0 = (double)cam[kCamT], t1 = (double)cam[kCamT + 1], t2 = (double)cam[kCamT + 2];
            const double w0 = p.weighted ? (double)score : 1.0;
            double wu = w0 * (fx * fx), wv = w0 * (fy * fy);
            if (pass > 0) {
                const double Xc = r00 * X0 + r01 * X1 + r02 * X2 + t0, Yc = r10 * X0 + r11 * X1 + r12 * X2 + t1, Zc = r20 * X0 + r21 * X1 + r22 * X2 + t2;
                if (!(Zc > 0.0)) behind = true;
                const double du = fx * (Xc / Zc - x), dv = fy * (Yc / Zc - y);
                const double rho = du * du + dv * dv;
                if (last) {
                    num = num + w0 * rho;
                    den = den + w0;
                    sx[v * TRI_TILE] = sqrt(rho);
                    continue;
                }
                const double g = w0 / (1.0 + rho / d2), z2 = Zc * Zc;
                wu = g * (fx * fx) / z2;
                wv = g * (fy * fy) / z2;
            }
            tri_row(s, wu, x * r20 - r00, x * r21 - r01, x * r22 - r02, t0 - x * t2);
            tri_row(s, wv, y * r20 - r10, y * r21 - r11, y * r22 - r12, t1 - y * t2);
        }
        if (last) break;
        // A = L D L^T in the order 0, 1, 2 without exchanges; every pivot is held against the trace
        const double floor_ = kTriPivot * (s.a00 + s.a11 + s.a22);
        const double d0 = s.a00;
        const double l10 = s.a01 / d0, l20 = s.a02 / d0;
        const double d1 = s.a11 - l10 * s.a01;
        const double m12 = s.a12 - l10 * s.a02;
        const double l21 = m12 / d1;
        const double dd2 = s.a22 - l20 * s.a02 - l21 * m12;
        if (!(d0 > floor_) || !(d1 > floor_) || !(dd2 > floor_)) flat = true;
        const double c1 = s.b1 - l10 * s.b0;
        const double c2 = s.b2 - l20 * s.b0 - l21 * c1;
        X2 = c2 / dd2;
        X1 = c1 / d1 - l21 * X2;
        X0 = s.b0 / d0 - l10 * X1 - l20 * X2;
        if (!(fabs(X0) <= kTriHuge) || !(fabs(X1) <= kTriHuge) || !(fabs(X2) <= kTriHuge)) flat = true;
    }
    X[0] = X0, X[1] = X1, X[2] = X2;
    res = sqrt(num / den);
    return n_used < p.min_views ? 1 : (flat ? 2 : (behind ? 3 : 0));
}

template <bool PER_FRAME>
__global__ __launch_bounds__(TRI_TILE) void k_keypoints_triangulate(const float* __restrict__ keypoints, int C, int64_t M, int ppf,
                                                                    const float* __restrict__ cameras, KasfTriangulate p, float* __restrict__ points,
                                                                    float* __restrict__ residual, unsigned char* __restrict__ used,
                                                                    unsigned char* __restrict__ state, float* __restrict__ view_residual) {
    KASF_DYNAMIC_LDS(sm);
    double* s_x = reinterpret_cast<double*>(sm);                // [C][TRI_TILE]
    double* s_y = s_x + C * TRI_TILE;                           // [C][TRI_TILE]
    float* s_w = reinterpret_cast<float*>(s_y + C * TRI_TILE);  // [C][TRI_TILE]: the score, NaN where the view is not usable
    float* s_stage = s_w + C * TRI_TILE;                        // [TRI_TILE][3]: a view's records in, the points out
    float* s_cam = s_stage + TRI_TILE_FLOATS;                   // [C][21]: a static rig
    const int tid = threadIdx.x;
    const int64_t F = M / ppf, tiles = (M + TRI_TILE - 1) / TRI_TILE;
    if (!PER_FRAME)
        for (int i = tid; i < C * kCamFloats; i += TRI_TILE) s_cam[i] = cameras[i];      // read behind the first barrier below
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * TRI_TILE, n = first + tid;
        const int count = (int)(M - first < TRI_TILE ? M - first : TRI_TILE);
        const bool live = tid < count;
        // view 0's camera row of this lane's point, and the floats from one view's row to the next
        const float* cam0 = PER_FRAME ? cameras + (live ? n / ppf : 0) * kCamFloats : s_cam;
        const int64_t cam_step = PER_FRAME ? F * kCamFloats : kCamFloats;
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const float* src = keypoints + first * 3;
        bool vec = count == TRI_TILE && tri_aligned16(src);
        tile_fetch<TRI_TILE>(src, count, vec, r);
        int n_used = 0;
        for (int v = 0; v < C; ++v) {                           // step 1 and the undistortion, view by view
            tile_stash<TRI_TILE>(s_stage, count, vec, r);
            __syncthreads();
            if (v + 1 < C) {
                src = keypoints + ((int64_t)(v + 1) * M + first) * 3;
                vec = count == TRI_TILE && tri_aligned16(src);
                tile_fetch<TRI_TILE>(src, count, vec, r);
            }
            if (live) {
                const float* k = s_stage + tid * 3;
                const float* cam = cam0 + v * cam_step;
                const bool ok = joint_usable<2>(k, true, p.min_score) && camera_finite(cam, kCamFloats);
                double x = 0.0, y = 0.0;
                if (ok) camera_undistort(cam, k[0], k[1], p.undistort_iterations, x, y);
                s_x[v * TRI_TILE + tid] = x;
                s_y[v * TRI_TILE + tid] = y;
                s_w[v * TRI_TILE + tid] = ok ? k[2] : tri_nan();
                n_used += ok ? 1 : 0;
            }
            __syncthreads();                                    // the next view overwrites the staging tile
        }
        if (live) {
            double X[3], res;
            const int st = tri_point(s_x + tid, s_y + tid, s_w + tid, cam0, cam_step, C, n_used, p, X, res);
            s_stage[tid * 3] = st == 0 ? (float)X[0] : tri_nan();
            s_stage[tid * 3 + 1] = st == 0 ? (float)X[1] : tri_nan();
            s_stage[tid * 3 + 2] = st == 0 ? (float)X[2] : tri_nan();
            if (residual != nullptr) residual[n] = st == 0 ? (float)res : tri_nan();
            if (used != nullptr) used[n] = (unsigned char)n_used;
            if (state != nullptr) state[n] = (unsigned char)st;
            if (view_residual != nullptr)
                for (int v = 0; v < C; ++v) {
                    const float score = s_w[v * TRI_TILE + tid];
                    view_residual[(int64_t)v * M + n] = st == 0 && score == score ? (float)s_x[v * TRI_TILE + tid] : tri_nan();
                }
        }
        __syncthreads();
        tile_store<TRI_TILE>(s_stage, count, points + first * 3);
        __syncthreads();                                        // the next pass overwrites the staging tile
    }
}

__global__ __launch_bounds__(UND_TILE) void k_keypoints_undistort(const float* __restrict__ keypoints, int64_t M, int ppf, const float* __restrict__ camera,
                                                                  int camera_per_frame, int rounds, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[UND_TILE_FLOATS];
    const int tid = threadIdx.x;
    const int64_t tiles = (M + UND_TILE - 1) / UND_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * UND_TILE, n = first + tid;
        const int count = (int)(M - first < UND_TILE ? M - first : UND_TILE);
        const float* src = keypoints + first * 3;
        const bool vec = count == UND_TILE && tri_aligned16(src);
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        tile_fetch<UND_TILE>(src, count, vec, r);
        tile_stash<UND_TILE>(tile, count, vec, r);
        __syncthreads();
        if (tid < count) {
            float* k = tile + tid * 3;
            const float* cam = camera + (camera_per_frame ? (n / ppf) * kCamLensFloats : 0);
            if (joint_usable<2>(k, false, 0.0f) && camera_finite(cam, kCamLensFloats)) {
                double x, y;
                camera_undistort(cam, k[0], k[1], rounds, x, y);
                k[0] = (float)((double)cam[kCamFx] * x + (double)cam[kCamCx]);
                k[1] = (float)((double)cam[kCamFy] * y + (double)cam[kCamCy]);
            }
        }
        __syncthreads();
        tile_store<UND_TILE>(tile, count, out + first * 3);
        __syncthreads();                                        // the next pass overwrites the tile
    }
}

}  // namespace

// the LDS a triangulation workgroup asks for: two fp64 planes and a score plane [C][TRI_TILE], the staging tile, the static rig's rows
static size_t tri_lds_bytes(int C) { return (size_t)C * TRI_TILE * 20 + TRI_TILE_FLOATS * 4 + (size_t)C * kCamFloats * 4; }

// the arguments as the entry point checked them: keypoints [C][M][3], cameras [C][21] or [C][M / ppf][21]; residual, used, state, view_residual may be null
void kasf_launch_keypoints_triangulate(hipStream_t s, const float* keypoints, int C, int64_t M, int ppf, const float* cameras, int cameras_per_frame,
                                       const KasfTriangulate& p, float* points, float* residual, unsigned char* used, unsigned char* state,
                                       float* view_residual) {
    if (M <= 0) return;
    const int64_t g = (M + TRI_TILE - 1) / TRI_TILE;
    const dim3 grid((unsigned)(g > 65536 ? 65536 : g));
    if (cameras_per_frame)
        hipLaunchKernelGGL(k_keypoints_triangulate<true>, grid, dim3(TRI_TILE), tri_lds_bytes(C), s, keypoints, C, M, ppf, cameras, p, points, residual, used,
                           state, view_residual);
    else
        hipLaunchKernelGGL(k_keypoints_triangulate<false>, grid, dim3(TRI_TILE), tri_lds_bytes(C), s, keypoints, C, M, ppf, cameras, p, points, residual, used,
                           state, view_residual);
}

// camera [9] or [M / ppf][9]
void kasf_launch_keypoints_undistort(hipStream_t s, const float* keypoints, int64_t M, int ppf, const float* camera, int camera_per_frame, int rounds,
                                     float* out) {
    if (M <= 0) return;
    const int64_t g = (M + UND_TILE - 1) / UND_TILE;
    hipLaunchKernelGGL(k_keypoints_undistort, dim3((unsigned)(g > 65536 ? 65536 : g)), dim3(UND_TILE), 0, s, keypoints, M, ppf, camera, camera_per_frame, rounds,
                       out);
}
