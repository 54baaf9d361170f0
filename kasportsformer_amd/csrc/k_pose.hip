// The two ends of the lift that the demo does on the host (kasf.h, kasf_coco_h36m / kasf_pose_world):
//   in:  COCO-17 detector keypoints -> the Human3.6M-17 layout the model was trained on (h36m_coco_format / coco_h36m, demo/lib/preprocess.py:10-69)
//   out: camera-space poses -> world space, feet on the floor, unit scale (camera_to_world / qrot, demo/lib/utils.py:55-73; demo/demo.py:242-248)
// Both move 51 floats per frame in and 51 out: HBM-bound.  A frame's outputs mix up to five of its inputs (and, for the world step, all 51 through two
// reductions), so a workgroup stages a tile of POSE_TILE frames in LDS: the global loads and stores are one float4 per lane on consecutive addresses
// (one fp32 per lane where a pointer is not 16-byte aligned and in the last, partial tile), and between them lane i works on frame i of the tile alone:
// its 51 floats sit at LDS stride 51, an odd number of banks, so the 32 lanes of an LDS access never share one.  The joint recipes are written out
// (no table, no divergent index), the reductions are sequential in registers (no LDS atomics), and every expression keeps the reference's operation
// order in fp32 -- the library is built with -ffp-contract=off and a correctly rounded divide -- so the results are the reference's bit for bit.
#include "kernels.h"

namespace {

constexpr int POSE_TILE = 128;                                  // frames per workgroup pass = threads per workgroup; 128 * 204 B = 25.5 KiB of LDS
constexpr int POSE_TILE_FLOATS = POSE_TILE * 51;                // 6,528: a multiple of 4, so every full tile starts 16-byte aligned when the array does

// frames [first, first + count) of src -> LDS tile (and back): VEC = the float4 form, for full tiles of 16-byte aligned arrays
template <bool VEC>
__device__ inline void tile_load(const float* __restrict__ src, int64_t first, int count, float* tile) {
    if (VEC && count == POSE_TILE) {
        const float4* s4 = reinterpret_cast<const float4*>(src + first * 51);
        float4* t4 = reinterpret_cast<float4*>(tile);
        for (int i = threadIdx.x; i < POSE_TILE_FLOATS / 4; i += POSE_TILE) t4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < count * 51; i += POSE_TILE) tile[i] = src[first * 51 + i];
    }
}
template <bool VEC>
__device__ inline void tile_store(const float* tile, int64_t first, int count, float* __restrict__ dst) {
    if (VEC && count == POSE_TILE) {
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        float4* d4 = reinterpret_cast<float4*>(dst + first * 51);
        for (int i = threadIdx.x; i < POSE_TILE_FLOATS / 4; i += POSE_TILE) d4[i] = t4[i];
    } else {
        for (int i = threadIdx.x; i < count * 51; i += POSE_TILE) dst[first * 51 + i] = tile[i];
    }
}

// One frame in place, f[17][3] = COCO x, y, score -> H36M x, y, score.  COCO: 0 nose, 1-2 eyes, 3-4 ears, 5-6 shoulders, 7-8 elbows, 9-10 wrists,
// 11-12 hips, 13-14 knees, 15-16 ankles.  H36M: 0 pelvis, 1-3 right leg, 4-6 left leg, 7 spine, 8 thorax, 9 neck/nose, 10 head, 11-13 left arm,
// 14-16 right arm.  np.mean(..., dtype=float32) is the left-to-right sum divided by the count.
__device__ inline void coco_frame_to_h36m(float* f) {
    float k[17][3];
#pragma unroll
    for (int j = 0; j < 17; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) k[j][c] = f[3 * j + c];
    float h[17][3];
    // preprocess.py:25 (and :58 for the scores): the thirteen joints both layouts have
    constexpr int h36m_of[13] = {9, 11, 14, 12, 15, 13, 16, 4, 1, 5, 2, 6, 3}, coco_of[13] = {0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
#pragma unroll
    for (int i = 0; i < 13; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) h[h36m_of[i]][c] = k[coco_of[i]][c];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float shoulders = (k[5][c] + k[6][c]) / 2.0f;
        h[0][c] = (k[11][c] + k[12][c]) / 2.0f;                                            // :21 pelvis
        h[7][c] = (((k[5][c] + k[6][c]) + k[11][c]) + k[12][c]) / 4.0f;                    // :22 spine
        h[8][c] = shoulders + (k[0][c] - shoulders) / 3.0f;                                // :18-19 thorax
        h[9][c] = k[0][c] - (k[0][c] - shoulders) / 4.0f;                                  // :27 neck: reads the nose copied by :25
    }
    h[10][0] = (((k[1][0] + k[2][0]) + k[3][0]) + k[4][0]) / 4.0f;                         // :16 head x: eyes and ears
    h[10][1] = (k[1][1] + k[2][1]) - k[0][1];                                              // :17 head y
    h[7][0] = h[7][0] + 2.0f * (h[7][0] - (h[0][0] + h[8][0]) / 2.0f);                     // :28 spine x, from pelvis and thorax (factor 2)
    h[8][1] = h[8][1] - (((k[1][1] + k[2][1]) / 2.0f - k[0][1]) * 2.0f) / 3.0f;            // :29 thorax y, after :28
    // preprocess.py:59-62: the scores of the four joints COCO lacks
    h[0][2] = (k[11][2] + k[12][2]) / 2.0f;
    h[8][2] = (k[5][2] + k[6][2]) / 2.0f;
    h[7][2] = (h[0][2] + h[8][2]) / 2.0f;
    h[10][2] = (((k[1][2] + k[2][2]) + k[3][2]) + k[4][2]) / 4.0f;
#pragma unroll
    for (int j = 0; j < 17; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) f[3 * j + c] = h[j][c];
}

template <bool VEC>
__global__ __launch_bounds__(POSE_TILE) void k_coco_h36m(const float* __restrict__ coco, int64_t frames, float* __restrict__ h36m) {
    __shared__ __attribute__((aligned(16))) float tile[POSE_TILE_FLOATS];
    const int64_t tiles = (frames + POSE_TILE - 1) / POSE_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * POSE_TILE;
        const int count = (int)(frames - first < POSE_TILE ? frames - first : POSE_TILE);
        tile_load<VEC>(coco, first, count, tile);
        __syncthreads();
        if ((int)threadIdx.x < count) coco_frame_to_h36m(tile + threadIdx.x * 51);
        __syncthreads();
        tile_store<VEC>(tile, first, count, h36m);
        __syncthreads();                                        // the next pass overwrites the tile
    }
}

// One frame in place, f[17][3] camera space -> world space: qrot's v + 2 * (q0 * (q x v) + q x (q x v)) (torch.cross's a1 b2 - a2 b1, ...) plus t;
// floor: minus the frame's smallest z (demo.py:246); unit: all 51 values divided by their largest (demo.py:247-248; a largest value of 0 divides by 0
// as the reference does).  min / max pass a NaN on, as numpy's do.
__device__ inline void frame_to_world(float* f, float q0, float q1, float q2, float q3, float t0, float t1, float t2, int floor, int unit) {
    float v[17][3];
#pragma unroll
    for (int j = 0; j < 17; ++j) {
        const float x = f[3 * j], y = f[3 * j + 1], z = f[3 * j + 2];
        const float ux = q2 * z - q3 * y, uy = q3 * x - q1 * z, uz = q1 * y - q2 * x;
        const float wx = q2 * uz - q3 * uy, wy = q3 * ux - q1 * uz, wz = q1 * uy - q2 * ux;
        v[j][0] = (x + 2.0f * (q0 * ux + wx)) + t0;
        v[j][1] = (y + 2.0f * (q0 * uy + wy)) + t1;
        v[j][2] = (z + 2.0f * (q0 * uz + wz)) + t2;
    }
    if (floor) {
        float lo = v[0][2];
#pragma unroll
        for (int j = 1; j < 17; ++j) lo = (v[j][2] < lo || v[j][2] != v[j][2]) ? v[j][2] : lo;
#pragma unroll
        for (int j = 0; j < 17; ++j) v[j][2] = v[j][2] - lo;
    }
    if (unit) {
        float hi = v[0][0];
#pragma unroll
        for (int i = 1; i < 51; ++i) {
            const float a = v[i / 3][i % 3];
            hi = (a > hi || a != a) ? a : hi;
        }
#pragma unroll
        for (int i = 0; i < 51; ++i) v[i / 3][i % 3] = v[i / 3][i % 3] / hi;
    }
#pragma unroll
    for (int j = 0; j < 17; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) f[3 * j + c] = v[j][c];
}

template <bool VEC>
__global__ __launch_bounds__(POSE_TILE) void k_pose_world(const float* __restrict__ poses, int64_t frames, float q0, float q1, float q2, float q3, float t0,
                                                          float t1, float t2, int floor, int unit, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[POSE_TILE_FLOATS];
    const int64_t tiles = (frames + POSE_TILE - 1) / POSE_TILE;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t first = t * POSE_TILE;
        const int count = (int)(frames - first < POSE_TILE ? frames - first : POSE_TILE);
        tile_load<VEC>(poses, first, count, tile);
        __syncthreads();
        if ((int)threadIdx.x < count) frame_to_world(tile + threadIdx.x * 51, q0, q1, q2, q3, t0, t1, t2, floor, unit);
        __syncthreads();
        tile_store<VEC>(tile, first, count, out);
        __syncthreads();
    }
}

inline unsigned tiles_grid(int64_t frames) {
    const int64_t g = (frames + POSE_TILE - 1) / POSE_TILE;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
inline bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace

void kasf_launch_coco_h36m(hipStream_t s, const float* coco, int64_t frames, float* h36m) {
    if (frames <= 0) return;
    if (aligned16(coco, h36m)) hipLaunchKernelGGL(k_coco_h36m<true>, dim3(tiles_grid(frames)), dim3(POSE_TILE), 0, s, coco, frames, h36m);
    else hipLaunchKernelGGL(k_coco_h36m<false>, dim3(tiles_grid(frames)), dim3(POSE_TILE), 0, s, coco, frames, h36m);
}

void kasf_launch_pose_world(hipStream_t s, const float* poses, int64_t frames, const float* q, const float* t, int floor, int unit, float* out) {
    if (frames <= 0) return;
    if (aligned16(poses, out))
        hipLaunchKernelGGL(k_pose_world<true>, dim3(tiles_grid(frames)), dim3(POSE_TILE), 0, s, poses, frames, q[0], q[1], q[2], q[3], t[0], t[1], t[2], floor,
                           unit, out);
    else
        hipLaunchKernelGGL(k_pose_world<false>, dim3(tiles_grid(frames)), dim3(POSE_TILE), 0, s, poses, frames, q[0], q[1], q[2], q[3], t[0], t[1], t[2], floor,
                           unit, out);
}
