// Where a lifted pose stands in front of the camera (kasf.h, kasf_pose_place): the root translation T that makes a root-relative pose re-project onto its 2-D
// keypoints through a pinhole camera, a weighted linear least-squares fit per frame with Cauchy re-weighting, and optionally a metric scale from a bone table.
// place_frame is the one statement of the rule's arithmetic: every line is the rounded fp64 operation(s) kasf.h names, left to right (-ffp-contract=off, a
// correctly rounded divide and square root), and the results are rounded to fp32 once, at the store.
//
// One launch, 633 B per frame (204 pose in, 204 keypoints in, 204 pose out, 21 of root, residual, scale and state): HBM-bound.  As in k_pose.hip a workgroup
// stages a tile of PLACE_TILE frames of both arrays in LDS -- global loads and stores are one float4 per lane on consecutive addresses where all three arrays are
// 16-byte aligned, one fp32 per lane otherwise and in the last, partial tile -- and lane i then owns frame i of the tile: its rows sit at LDS stride 51, an odd
// number of banks, so the lanes of an LDS access never share one.  A pass of the fit walks the 17 joints out of LDS (nothing is indexed in registers: no
// scratch) with its nine accumulators in fp64 registers; the placed pose overwrites the pose tile and leaves as whole rows.  No atomics, no transcendental (a
// square root is none), every output element is written by one lane: the same bits from run to run, and a frame's result does not depend on its neighbours.
//
// PLACE_TILE is 64, one wavefront per workgroup: two tiles are 25.5 KiB of static LDS.  LDS is what bounds the occupancy whatever the tile, 408 B per lane: a
// CU's 160 KiB hold six workgroups, six wavefronts, and 128-frame tiles (51 KiB, three workgroups of two wavefronts) would give the same six with half as many
// workgroups to spread over the chip: one 18,000-frame track is 282 tiles of 64 for 256 CUs, but only 141 of 128 ("camera-space placement").
#include "kernels.h"
#include "bone_table.h"
#include "one_euro.h"

namespace {

constexpr int PLACE_TILE = 64;                                  // frames per workgroup pass = threads per workgroup
constexpr int PLACE_TILE_FLOATS = PLACE_TILE * 51;              // 3,264: a multiple of 4, so every full tile starts 16-byte aligned when the array does
constexpr double kPlaceHuge = 1.7976931348623157e308;           // the largest finite double: v <= kPlaceHuge is false for a NaN and for +infinity
constexpr double kPlacePivot = 1e-9;                            // the pivot test of kasf.h: D > kPlacePivot * Sq

// frames [first, first + count) of src -> LDS tile (and back): VEC = the float4 form, for full tiles of 16-byte aligned arrays
template <bool VEC>
__device__ inline void place_tile_load(const float* __restrict__ src, int64_t first, int count, float* tile) {
    if (VEC && count == PLACE_TILE) {
        const float4* s4 = reinterpret_cast<const float4*>(src + first * 51);
        float4* t4 = reinterpret_cast<float4*>(tile);
        for (int i = threadIdx.x; i < PLACE_TILE_FLOATS / 4; i += PLACE_TILE) t4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < count * 51; i += PLACE_TILE) tile[i] = src[first * 51 + i];
    }
}
template <bool VEC>
__device__ inline void place_tile_store(const float* tile, int64_t first, int count, float* __restrict__ dst) {
    if (VEC && count == PLACE_TILE) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* d4 = reinterpret_cast<float4*>(dst + first * 51);
        for (int i = threadIdx.x; i < PLACE_TILE_FLOATS / 4; i += PLACE_TILE) d4[i] = t4[i];
    } else {
        for (int i = threadIdx.x; i < count * 51; i += PLACE_TILE) dst[first * 51 + i] = tile[i];
    }
}

__device__ inline bool place_finite(float v) { return fabsf(v) <= 3.4028235e38f; }               // false for a NaN and for an infinity
__device__ inline bool place_positive(double v) { return v > 0.0 && v <= kPlaceHuge; }           // finite and positive
__device__ inline float place_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }

// step 1 of the rule: the keypoint passes the One-Euro step's own test (two channels and a score) and the joint's three pose values are finite
__device__ inline bool place_usable(const float* P, const float* K, int j, float min_score) {
    return joint_usable<2>(K + 3 * j, true, min_score) && place_finite(P[3 * j]) && place_finite(P[3 * j + 1]) && place_finite(P[3 * j + 2]);
}

// One frame.  P: its pose [17][3], replaced by the placed pose; K: its keypoints [17][3]; cam: fx, fy, cx, cy; L: the bone table [16] or null.
// root3, residual, scale: where this frame's values go (any may be null).  Returns the state.
__device__ inline int place_frame(float* P, const float* K, const float* __restrict__ cam, const float* __restrict__ L, const KasfPlace& p,
                                  float* __restrict__ root3, float* __restrict__ residual, float* __restrict__ scale_out) {
    const double fx = (double)cam[0], fy = (double)cam[1], cx = (double)cam[2], cy = (double)cam[3];
    // step 2: the metric scale, computed whatever the state turns out to be
    double scale = 1.0;
    if (L != nullptr) {
        double sumL = 0.0, sumP = 0.0;
        for (int b = 0; b < 16; ++b) {
            const float Lb = L[b];
            if (Lb > 0.0f) {
                const int ch = b + 1, pa = bone_parent(b);
                const double dx = (double)P[3 * ch] - (double)P[3 * pa], dy = (double)P[3 * ch + 1] - (double)P[3 * pa + 1],
                             dz = (double)P[3 * ch + 2] - (double)P[3 * pa + 2];
                sumL = sumL + (double)Lb;
                sumP = sumP + sqrt((dx * dx + dy * dy) + dz * dz);
            }
        }
        scale = sumL / sumP;
    }
    // step 1: how many joints can be used
    int usable = 0;
    for (int j = 0; j < 17; ++j) usable += place_usable(P, K, j, p.min_score) ? 1 : 0;
    int state = usable < p.min_joints ? 1 : (place_positive(scale) ? 0 : 3);

    const double d2 = (double)p.delta * (double)p.delta;
    double Tx = 0.0, Ty = 0.0, Tz = 0.0, num = 0.0, den = 0.0;
    bool bad = false;                                           // a pivot failed, a T was not finite or a usable joint was not in front of the camera
    // steps 3 and 4: pass 0 fits with the initial weights, passes 1 .. iterations with the weights of the residuals at the T before, and the last pass only
    // measures: the residual at the final T
    for (int pass = 0; pass <= p.iterations + 1; ++pass) {
        const bool last = pass == p.iterations + 1;
        double S = 0.0, Sx = 0.0, Sy = 0.0, Sq = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int j = 0; j < 17; ++j) {
            if (!place_usable(P, K, j, p.min_score)) continue;
            const double px = (double)P[3 * j] * scale, py = (double)P[3 * j + 1] * scale, pz = (double)P[3 * j + 2] * scale;
            const double u = (double)K[3 * j], v = (double)K[3 * j + 1];
            const double w0 = p.weighted ? (double)K[3 * j + 2] : 1.0;
            double w = w0;
            if (pass > 0) {
                const double X = px + Tx, Y = py + Ty, Z = pz + Tz;
                if (!(Z > 0.0)) bad = true;
                const double du = (fx * (X / Z) + cx) - u, dv = (fy * (Y / Z) + cy) - v;
                const double r2 = du * du + dv * dv;
                if (last) {
                    num = num + w0 * r2;
                    den = den + w0;
                    continue;
                }
                w = w0 / (1.0 + r2 / d2);
            }
            const double xh = (u - cx) / fx, yh = (v - cy) / fy;
            const double q1 = xh * pz - px, q2 = yh * pz - py;
            S = S + w;
            Sx = Sx + w * xh;
            Sy = Sy + w * yh;
            Sq = Sq + w * (xh * xh + yh * yh);
            b0 = b0 + w * q1;
            b1 = b1 + w * q2;
            b2 = b2 + w * (xh * q1 + yh * q2);
        }
        if (last) break;
        // A = [[S, 0, -Sx], [0, S, -Sy], [-Sx, -Sy, Sq]], right-hand side (b0, b1, -b2): eliminate the first two unknowns, D is the third pivot
        const double D = Sq - (Sx * Sx + Sy * Sy) / S;
        if (!(S > 0.0) || !(D > kPlacePivot * Sq)) bad = true;
        Tz = ((Sx * b0 + Sy * b1) / S - b2) / D;
        Tx = (b0 + Sx * Tz) / S;
        Ty = (b1 + Sy * Tz) / S;
        if (!(fabs(Tx) <= kPlaceHuge) || !(fabs(Ty) <= kPlaceHuge) || !(fabs(Tz) <= kPlaceHuge)) bad = true;
    }
    if (state == 0 && bad) state = 2;
    // step 5
    if (state == 0) {
        for (int j = 0; j < 17; ++j) {
            P[3 * j] = (float)((double)P[3 * j] * scale + Tx);
            P[3 * j + 1] = (float)((double)P[3 * j + 1] * scale + Ty);
            P[3 * j + 2] = (float)((double)P[3 * j + 2] * scale + Tz);
        }
    } else {
        for (int i = 0; i < 51; ++i) P[i] = place_nan();
    }
    if (root3 != nullptr) {
        root3[0] = state == 0 ? (float)Tx : place_nan();
        root3[1] = state == 0 ? (float)Ty : place_nan();
        root3[2] = state == 0 ? (float)Tz : place_nan();
    }
    if (residual != nullptr) *residual = state == 0 ? (float)sqrt(num / den) : place_nan();
    if (scale_out != nullptr) *scale_out = (float)scale;
    return state;
}

template <bool VEC>
__global__ __launch_bounds__(PLACE_TILE) void k_pose_place(const float* __restrict__ poses, const float* __restrict__ keypoints, int64_t frames,
                                                           const float* __restrict__ camera, int camera_per_frame, const float* __restrict__ lengths,
                                                           int lengths_per_frame, KasfPlace p, float* __restrict__ out, float* __restrict__ root,
                                                           float* __restrict__ residual, float* __restrict__ scale, unsigned char* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) float tile_p[PLACE_TILE_FLOATS];
    __shared__ __attribute__((aligned(16))) float tile_k[PLACE_TILE_FLOATS];
    const int64_t tiles = (frames + PLACE_TILE - 1) / PLACE_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * PLACE_TILE;
        const int count = (int)(frames - first < PLACE_TILE ? frames - first : PLACE_TILE);
        place_tile_load<VEC>(poses, first, count, tile_p);
        place_tile_load<VEC>(keypoints, first, count, tile_k);
        __syncthreads();
        if ((int)threadIdx.x < count) {
            const int64_t f = first + threadIdx.x;
            const int st = place_frame(tile_p + threadIdx.x * 51, tile_k + threadIdx.x * 51, camera + (camera_per_frame ? f * 4 : 0),
                                       lengths != nullptr ? lengths + (lengths_per_frame ? f * 16 : 0) : nullptr, p, root != nullptr ? root + f * 3 : nullptr,
                                       residual != nullptr ? residual + f : nullptr, scale != nullptr ? scale + f : nullptr);
            if (state != nullptr) state[f] = (unsigned char)st;
        }
        __syncthreads();
        place_tile_store<VEC>(tile_p, first, count, out);
        __syncthreads();                                        // the next pass overwrites the tiles
    }
}

}  // namespace

// the parameters as the entry point checked them; camera [4] or [frames][4], lengths null, [16] or [frames][16]; root, residual, scale, state may be null
void kasf_launch_pose_place(hipStream_t s, const float* poses, const float* keypoints, int64_t frames, const float* camera, int camera_per_frame,
                            const float* lengths, int lengths_per_frame, const KasfPlace& p, float* out, float* root, float* residual, float* scale,
                            unsigned char* state) {
    if (frames <= 0) return;
    const int64_t g = (frames + PLACE_TILE - 1) / PLACE_TILE;
    const dim3 grid((unsigned)(g > 65536 ? 65536 : g));
    if (((((uintptr_t)poses | (uintptr_t)keypoints) | (uintptr_t)out) & 15) == 0)
        hipLaunchKernelGGL(k_pose_place<true>, grid, dim3(PLACE_TILE), 0, s, poses, keypoints, frames, camera, camera_per_frame, lengths, lengths_per_frame, p, out,
                           root, residual, scale, state);
    else
        hipLaunchKernelGGL(k_pose_place<false>, grid, dim3(PLACE_TILE), 0, s, poses, keypoints, frames, camera, camera_per_frame, lengths, lengths_per_frame, p,
                           out, root, residual, scale, state);
}
