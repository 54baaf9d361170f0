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
//
// Flip-tested heatmaps -> keypoints (kasf.h, kasf_heatmap_flip_keypoints): HRNet's FLIP_TEST / SHIFT_HEATMAP evaluation,
//   flip_back and the left / right pairs                                   demo/lib/hrnet/lib/utils/transforms.py:15-30
//   FLIP_TEST, POST_PROCESS, SHIFT_HEATMAP                                 demo/lib/hrnet/experiments/w48_384x288_adam_lr1e-3.yaml:119-121
// in front of the decode above, in one launch: merged[p][j][y][x] = (hm[p][j][y][x] + hmf[p][partner[j]][y][src_x(x)]) * 0.5f with
// src_x(x) = shift ? min(W - x, W - 1) : W - 1 - x, one fp32 add and one fp32 multiply, then the plain decode's rules on the merged values.  Both arrays
// are read once; merged is stored (fp32) only when the caller gives merged_out.
// MAPPING.  As the plain kernel: one wavefront owns one output map, HM_WAVES maps per workgroup, no LDS, no atomics, no barrier; lane l reads vector l, l + 64, ...
// of the direct map, 16 bytes each (VW = 4 fp32 or 8 fp16 / bf16 values), value k of vector v is map index v * VW + k; (value, index) pairs are reduced by six
// xor-shuffles under the same total order.  The flipped operand of a vector that starts at column x of row y is the row segment src_x(x + VW - 1) .. src_x(x) of
// the partner map, in descending order.  Three paths, the same arithmetic in each:
//   ROW   (both bases 16-byte aligned, a map a multiple of 16 bytes, W a multiple of VW)  a direct vector lies in one row and its mirror image W - x - VW ..
//         W - x - 1 is again an aligned vector of that row: one 16-byte load, read in reversed slot order.  Without shift that is all; with shift every slot moves
//         one element up, so slots 1 .. VW - 1 serve and the value above the vector, element min(W - x, W - 1) of the row (for x = 0 the clamp: slot VW - 1 once
//         more), comes from one element load of a line the neighbouring lane streams in the same instruction.  The 64 lanes of a load instruction cover one
//         contiguous span of both maps.
//   SPLIT (aligned as above, W not a multiple of VW: 4 x 6 fp32)  vectors straddle row ends: the direct operand stays on 16-byte loads, the flipped one is read
//         element by element.
//   ELEM  (a base not 16-byte aligned, or a map not a multiple of 16 bytes: 33 x 31, 5 x 3)  both operands element by element, VW = 1.
// Lane 0 then reads the four merged neighbours of the maximum (eight loads, all just streamed), refines, and applies the crop's inverse affine in fp64.
#include "kernels.h"
#include "crop_geom.h"

#include <climits>

namespace {

constexpr int HM_WAVES = 4;                                     // maps per workgroup = wavefronts per workgroup
constexpr int HM_THREADS = HM_WAVES * 64;
constexpr int ELEM = 0, SPLIT = 1, ROW = 2;                     // the flip kernel's paths

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

struct Best {
    float v;
    int i;
};

// the 64 lanes' pairs -> the wave's first pair under comes_first, in every lane (by value: a by-reference form changed the SPLIT loop's registers)
__device__ inline Best wave_first(float bv, int bi) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(bv, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (comes_first(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    return {bv, bi};
}

// What lane 0 does with the first pair (bv, bi) of map m, a joint of `person`: at(row, col) is the decoded map's value at index row + col, row being the index
// of a row's first element -- the flipped operand mirrors the column only, so it needs the two apart (one index would cost it a division per neighbour, which
// the one-wave-per-map launch at a team's worth of persons shows).  The pointers into geom and out are formed here, behind the neighbour loads.
template <class At>
__device__ inline void finish(float bv, int bi, int64_t m, int64_t person, int H, int W, int refine, const float* geom, int geom_kind, double aspect,
                              float* out, At at) {
    // get_max_preds (inference.py:21-49): x = idx % W, y = idx / W, times the mask "maxval > 0" (false for a NaN)
    int px = bi % W, py = bi / W;
    if (!(bv > 0.0f)) px = py = 0;
    float x = (float)px, y = (float)py;
    // POST_PROCESS (inference.py:59-72): strict bounds on both sides, differences and the quarter step in fp32
    if (refine && 1 < px && px < W - 1 && 1 < py && py < H - 1) {
        const int row = py * W;
        x = x + sign_of(at(row, px + 1) - at(row, px - 1)) * 0.25f;
        y = y + sign_of(at(row + W, px) - at(row - W, px)) * 0.25f;
    }
    // the person's crop: center and scale[0] as fp32, given or from the box (box_to_center_scale), and transform_preds with rot = 0 (transforms.py:50-101):
    // three anchor points stored as fp32, the affine through them solved in fp64 (crop_geom.h, shared with k_crop.hip) and applied in fp64
    const KasfCropGeom cg = kasf_crop_geom(geom + person * 4, geom_kind, aspect, W);
    const float cx = cg.cx, cy = cg.cy;
    const double kx = cg.kx, ky = cg.ky;
    const double half_w = (double)W * 0.5, half_h = (double)H * 0.5;
    float* o = out + m * 3;
    o[0] = (float)((double)cx + ((double)x - half_w) * kx);
    o[1] = (float)((double)cy + ((double)y - half_h) * ky);
    o[2] = bv;
}

// a grid-stride loop over the maps, HM_WAVES per workgroup
inline dim3 hm_grid(int64_t maps) {
    const int64_t groups = (maps + HM_WAVES - 1) / HM_WAVES;
    return dim3((unsigned)(groups > (1 << 20) ? (1 << 20) : groups));
}

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
        const Best b = wave_first(bv, bi);
        if (lane != 0) continue;
        finish(b.v, b.i, m, m / 17, H, W, refine, geom, geom_kind, aspect, out, [&](int row, int col) { return Elem<E>::up(map[row + col]); });
    }
}

template <class E>
void launch(hipStream_t s, const void* hm, int64_t maps, int H, int W, const float* geom, int geom_kind, double aspect, int refine, float* out) {
    using T = typename Elem<E>::T;
    const int64_t map_bytes = (int64_t)H * W * (int64_t)sizeof(T);
    const bool vec = ((uintptr_t)hm & 15) == 0 && (map_bytes & 15) == 0;
    const dim3 grid = hm_grid(maps), block(HM_THREADS);
    if (vec) hipLaunchKernelGGL((k_heatmap_keypoints<E, true>), grid, block, 0, s, (const T*)hm, maps, H, W, geom, geom_kind, aspect, refine, out);
    else hipLaunchKernelGGL((k_heatmap_keypoints<E, false>), grid, block, 0, s, (const T*)hm, maps, H, W, geom, geom_kind, aspect, refine, out);
}

// the 17 partner joints, 5 bits each, by value in the kernel's arguments: joints 0-11 in lo, 12-16 in hi
struct Partner {
    unsigned long long lo, hi;
};
__device__ inline int partner_of(const Partner& p, int j) { return (int)((j < 12 ? p.lo >> (5 * j) : p.hi >> (5 * (j - 12))) & 31u); }

// column of the flipped map that column x of the merged map takes: flip_back, then HRNet's one-column shift (column 0 keeps its unshifted value)
__device__ inline int src_x(int x, int W, int shift) { return shift ? min(W - x, W - 1) : W - 1 - x; }

// map index of the flipped operand of map index i
__device__ inline int flipped_index(int i, int W, int shift) {
    const int y = (int)((unsigned)i / (unsigned)W);
    return y * W + src_x(i - y * W, W, shift);
}

__device__ inline float merge(float a, float b) { return (a + b) * 0.5f; }

struct alignas(16) Float4 {
    float e[4];
};

template <class E, int MODE>
__global__ __launch_bounds__(HM_THREADS) void k_heatmap_flip_keypoints(const typename Elem<E>::T* __restrict__ hm, const typename Elem<E>::T* __restrict__ hmf,
                                                                       int64_t maps, int H, int W, Partner partner, int shift,
                                                                       const float* __restrict__ geom, int geom_kind, double aspect, int refine,
                                                                       float* __restrict__ out, float* __restrict__ merged_out) {
    using T = typename Elem<E>::T;
    constexpr int VW = Elem<E>::VW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HW = H * W;                                       // <= 2^24 (checked by the entry point)
    for (int64_t m = (int64_t)blockIdx.x * HM_WAVES + wave; m < maps; m += (int64_t)gridDim.x * HM_WAVES) {   // the tail: a wave without a map leaves
        const int64_t person = m / 17;
        const T* __restrict__ map = hm + m * HW;
        const T* __restrict__ fmap = hmf + (person * 17 + partner_of(partner, (int)(m - person * 17))) * HW;
        float* __restrict__ mo = merged_out ? merged_out + m * HW : nullptr;
        float bv = -INFINITY;
        int bi = INT_MAX;
        if (MODE != ELEM) {
            struct alignas(16) Vec { T e[VW]; };
            const Vec* __restrict__ map_v = reinterpret_cast<const Vec*>(map);
            const Vec* __restrict__ fmap_v = reinterpret_cast<const Vec*>(fmap);
            const int nvec = HW / VW;
#pragma unroll 2
            for (int v = lane; v < nvec; v += 64) {
                const int i0 = v * VW;
                const Vec a = map_v[v];
                float f[VW];
                if (MODE == ROW) {
                    const int y = (int)((unsigned)i0 / (unsigned)W), x = i0 - y * W;
                    const int row = y * W, mirror = W - x - VW;                 // a multiple of VW: the aligned vector that holds columns W - x - VW .. W - x - 1
                    const Vec b = fmap_v[(row + mirror) / VW];
                    if (shift) {
                        f[0] = merge(Elem<E>::up(a.e[0]), Elem<E>::up(fmap[row + min(W - x, W - 1)]));
#pragma unroll
                        for (int k = 1; k < VW; ++k) f[k] = merge(Elem<E>::up(a.e[k]), Elem<E>::up(b.e[VW - k]));
                    } else {
#pragma unroll
                        for (int k = 0; k < VW; ++k) f[k] = merge(Elem<E>::up(a.e[k]), Elem<E>::up(b.e[VW - 1 - k]));
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < VW; ++k) f[k] = merge(Elem<E>::up(a.e[k]), Elem<E>::up(fmap[flipped_index(i0 + k, W, shift)]));
                }
#pragma unroll
                for (int k = 0; k < VW; ++k)
                    if (comes_first(f[k], i0 + k, bv, bi)) { bv = f[k]; bi = i0 + k; }
                if (mo) {
#pragma unroll
                    for (int q = 0; q < VW / 4; ++q) {
                        Float4 o;
#pragma unroll
                        for (int k = 0; k < 4; ++k) o.e[k] = f[q * 4 + k];
                        *reinterpret_cast<Float4*>(mo + i0 + q * 4) = o;
                    }
                }
            }
        } else {
#pragma unroll 2
            for (int i = lane; i < HW; i += 64) {
                const float f = merge(Elem<E>::up(map[i]), Elem<E>::up(fmap[flipped_index(i, W, shift)]));
                if (comes_first(f, i, bv, bi)) { bv = f; bi = i; }
                if (mo) mo[i] = f;
            }
        }
        const Best b = wave_first(bv, bi);
        if (lane != 0) continue;
        // the MERGED neighbours of the maximum; src_x depends on the column only, so the operand one row up or down is the same column of row -+ W
        finish(b.v, b.i, m, person, H, W, refine, geom, geom_kind, aspect, out,
               [&](int row, int col) { return merge(Elem<E>::up(map[row + col]), Elem<E>::up(fmap[row + src_x(col, W, shift)])); });
    }
}

template <class E>
void launch_flip(hipStream_t s, const void* hm, const void* hmf, int64_t maps, int H, int W, Partner partner, int shift, const float* geom, int geom_kind,
                 double aspect, int refine, float* out, float* merged_out) {
    using T = typename Elem<E>::T;
    const int64_t map_bytes = (int64_t)H * W * (int64_t)sizeof(T);
    const bool vec = (((uintptr_t)hm | (uintptr_t)hmf | (uintptr_t)merged_out) & 15) == 0 && (map_bytes & 15) == 0;
    const int mode = !vec ? ELEM : (W % Elem<E>::VW == 0 ? ROW : SPLIT);
    const dim3 grid = hm_grid(maps), block(HM_THREADS);
    const T* a = (const T*)hm;
    const T* b = (const T*)hmf;
    if (mode == ROW)
        hipLaunchKernelGGL((k_heatmap_flip_keypoints<E, ROW>), grid, block, 0, s, a, b, maps, H, W, partner, shift, geom, geom_kind, aspect, refine, out, merged_out);
    else if (mode == SPLIT)
        hipLaunchKernelGGL((k_heatmap_flip_keypoints<E, SPLIT>), grid, block, 0, s, a, b, maps, H, W, partner, shift, geom, geom_kind, aspect, refine, out, merged_out);
    else
        hipLaunchKernelGGL((k_heatmap_flip_keypoints<E, ELEM>), grid, block, 0, s, a, b, maps, H, W, partner, shift, geom, geom_kind, aspect, refine, out, merged_out);
}

}  // namespace

void kasf_launch_heatmap_keypoints(hipStream_t s, const void* hm, int dtype, int64_t n, int H, int W, const float* geom, int geom_kind, double aspect,
                                   int refine, float* out) {
    if (n <= 0) return;
    if (dtype == KASF_F32) launch<F32>(s, hm, n * 17, H, W, geom, geom_kind, aspect, refine, out);
    else if (dtype == KASF_F16) launch<F16>(s, hm, n * 17, H, W, geom, geom_kind, aspect, refine, out);
    else launch<BF16>(s, hm, n * 17, H, W, geom, geom_kind, aspect, refine, out);
}

void kasf_launch_heatmap_flip_keypoints(hipStream_t s, const void* hm, const void* hmf, int dtype, int64_t n, int H, int W, const int* partner, int shift,
                                        const float* geom, int geom_kind, double aspect, int refine, float* out, float* merged_out) {
    if (n <= 0) return;
    Partner p = {0, 0};
    for (int j = 0; j < 17; ++j) {
        if (j < 12) p.lo |= (unsigned long long)(partner[j] & 31) << (5 * j);
        else p.hi |= (unsigned long long)(partner[j] & 31) << (5 * (j - 12));
    }
    if (dtype == KASF_F32) launch_flip<F32>(s, hm, hmf, n * 17, H, W, p, shift, geom, geom_kind, aspect, refine, out, merged_out);
    else if (dtype == KASF_F16) launch_flip<F16>(s, hm, hmf, n * 17, H, W, p, shift, geom, geom_kind, aspect, refine, out, merged_out);
    else launch_flip<BF16>(s, hm, hmf, n * 17, H, W, p, shift, geom, geom_kind, aspect, refine, out, merged_out);
}
