// Pose-network heatmaps -> keypoints in image pixels (kasf.h, kasf_heatmap_keypoints): what the demo does on the host after HRNet
//   get_final_preds = get_max_preds + the quarter-pixel POST_PROCESS + transform_preds   demo/lib/hrnet/lib/utils/inference.py:21-82, transforms.py:50-101
//   box_to_center_scale                                                                  demo/lib/hrnet/lib/utils/utilitys.py:102-135
// One pass over n * 17 * H * W values: HBM-bound at hundreds of persons, launch- and latency-bound at a team's worth.
// MAPPING.  One wavefront owns one map, HM_WAVES maps per workgroup, no LDS, no atomics, no barrier: a map is contiguous, so lane l of a wave reads
// vector l, l + 64, l + 128, ... of it, 16 bytes each (VW = 4 fp32 or 8 fp16 / bf16 values) -- 1 KiB per wave instruction on consecutive addresses.
// Value k of vector v is map index v * VW + k.  A lane's indices only grow, so it keeps (value, index) of its best value under a strict "greater"; the
// 64 pairs are then reduced by six xor-shuffles under one total order -- a NaN before any number, a larger value before a smaller, a lower index before
// a higher among equals -- which is np.argmax's answer (first maximum, first NaN) whatever the lane a value was read by.  A lane that read nothing
// holds (-inf, INT_MAX) and loses to every real entry.  Arrays whose base is not 16-byte aligned, or whose maps are not a multiple of 16 bytes (33 x 31,
// 5 x 3), take the same kernel with VW = 1.  Lane 0 of the wave then reads the four neighbours of the maximum (just streamed: L2-hot), refines, derives
// the person's crop geometry and applies the inverse crop affine in fp64: 2 of the 34 coordinates of a person.  The library is built with
// -ffp-contract=off, so every expression below rounds where the reference's numpy expression rounds.
#include "kernels.h"
#include "crop_geom.h"

#include <climits>

namespace {

constexpr int HM_WAVES = 4;                                     // maps per workgroup = wavefronts per workgroup
constexpr int HM_THREADS = HM_WAVES * 64;

struct F32 {};                                                  // element tags: how 16 bytes (or one element) become fp32 values, exactly
struct F16 {};
struct BF16 {};
template <class E> struct Elem;
template <> struct Elem<F32> {
    using T = float;
    static constexpr int VW = 4;
    static __device__ inline float up(float v) { return v; }
};
template <> struct Elem<F16> {
    using T = _Float16;
    static constexpr int VW = 8;
    static __device__ inline float up(_Float16 v) { return (float)v; }
};
template <> struct Elem<BF16> {
    using T = unsigned short;
    static constexpr int VW = 8;
    static __device__ inline float up(unsigned short v) { return __uint_as_float((unsigned)v << 16); }
};

// does candidate (cv, ci) come before (bv, bi)?  NaN first, then the larger value, then the lower index
__device__ inline bool comes_first(float cv, int ci, float bv, int bi) {
    const bool cn = cv != cv;
    if (bv != bv) return cn && ci < bi;
    return cn || cv > bv || (cv == bv && ci < bi);
}

// np.sign on one fp32 value: -1, 0, +1, and a NaN stays a NaN
__device__ inline float sign_of(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : (d == 0.0f ? 0.0f : d)); }

template <class E, bool VEC>
__global__ __launch_bounds__(HM_THREADS) void k_heatmap_keypoints(const typename Elem<E>::T* __restrict__ hm, int64_t maps, int H, int W,
                                                                  const float* __restrict__ geom, int geom_kind, double aspect, int refine,
                                                                  float* __restrict__ out) {
    using T = typename Elem<E>::T;
    constexpr int VW = Elem<E>::VW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HW = H * W;                                       // <= 2^24 (checked by the entry point)
    for (int64_t m = (int64_t)blockIdx.x * HM_WAVES + wave; m < maps; m += (int64_t)gridDim.x * HM_WAVES) {   // the tail: a wave without a map leaves
        const T* __restrict__ map = hm + m * HW;
        float bv = -INFINITY;
        int bi = INT_MAX;
        if (VEC) {
            struct alignas(16) Vec { T e[VW]; };
            const Vec* __restrict__ map_v = reinterpret_cast<const Vec*>(map);
            const int nvec = HW / VW;
#pragma unroll 4
            for (int v = lane; v < nvec; v += 64) {
                const Vec x = map_v[v];
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float f = Elem<E>::up(x.e[k]);
                    if (comes_first(f, v * VW + k, bv, bi)) { bv = f; bi = v * VW + k; }
                }
            }
        } else {
#pragma unroll 4
            for (int i = lane; i < HW; i += 64) {
                const float f = Elem<E>::up(map[i]);
                if (comes_first(f, i, bv, bi)) { bv = f; bi = i; }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(bv, d, 64);
            const int oi = __shfl_xor(bi, d, 64);
            if (comes_first(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane != 0) continue;
        // get_max_preds (inference.py:21-49): x = idx % W, y = idx / W, times the mask "maxval > 0" (false for a NaN)
        int px = bi % W, py = bi / W;
        if (!(bv > 0.0f)) px = py = 0;
        float x = (float)px, y = (float)py;
        // POST_PROCESS (inference.py:59-72): strict bounds on both sides, differences and the quarter step in fp32
        if (refine && 1 < px && px < W - 1 && 1 < py && py < H - 1) {
            const T* c = map + py * W + px;
            x = x + sign_of(Elem<E>::up(c[1]) - Elem<E>::up(c[-1])) * 0.25f;
            y = y + sign_of(Elem<E>::up(c[W]) - Elem<E>::up(c[-W])) * 0.25f;
        }
        // the person's crop: center and scale[0] as fp32, given or from the box (box_to_center_scale), and transform_preds with rot = 0 (transforms.py:50-101):
        // three anchor points stored as fp32, the affine through them solved in fp64 (crop_geom.h, shared with k_crop.hip) and applied in fp64
        const KasfCropGeom cg = kasf_crop_geom(geom + (m / 17) * 4, geom_kind, aspect, W);
        const float cx = cg.cx, cy = cg.cy;
        const double kx = cg.kx, ky = cg.ky;
        const double half_w = (double)W * 0.5, half_h = (double)H * 0.5;
        float* o = out + m * 3;
        o[0] = (float)((double)cx + ((double)x - half_w) * kx);
        o[1] = (float)((double)cy + ((double)y - half_h) * ky);
        o[2] = bv;
    }
}

template <class E>
void launch(hipStream_t s, const void* hm, int64_t maps, int H, int W, const float* geom, int geom_kind, double aspect, int refine, float* out) {
    using T = typename Elem<E>::T;
    const int64_t map_bytes = (int64_t)H * W * (int64_t)sizeof(T);
    const bool vec = ((uintptr_t)hm & 15) == 0 && (map_bytes & 15) == 0;
    const int64_t groups = (maps + HM_WAVES - 1) / HM_WAVES;
    const dim3 grid((unsigned)(groups > (1 << 20) ? (1 << 20) : groups)), block(HM_THREADS);
    if (vec) hipLaunchKernelGGL((k_heatmap_keypoints<E, true>), grid, block, 0, s, (const T*)hm, maps, H, W, geom, geom_kind, aspect, refine, out);
    else hipLaunchKernelGGL((k_heatmap_keypoints<E, false>), grid, block, 0, s, (const T*)hm, maps, H, W, geom, geom_kind, aspect, refine, out);
}

}  // namespace

void kasf_launch_heatmap_keypoints(hipStream_t s, const void* hm, int dtype, int64_t n, int H, int W, const float* geom, int geom_kind, double aspect,
                                   int refine, float* out) {
    if (n <= 0) return;
    if (dtype == KASF_F32) launch<F32>(s, hm, n * 17, H, W, geom, geom_kind, aspect, refine, out);
    else if (dtype == KASF_F16) launch<F16>(s, hm, n * 17, H, W, geom, geom_kind, aspect, refine, out);
    else launch<BF16>(s, hm, n * 17, H, W, geom, geom_kind, aspect, refine, out);
}
