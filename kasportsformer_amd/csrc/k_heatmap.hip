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

// ---- DARK / UDP sub-pixel decode (kasf.h, kasf_heatmap_decode) ----
//   DARK      Zhang et al., CVPR 2020: blur the map, take its logarithm, one Newton step from the argmax (mmpose's post_process = 'unbiased')
//   DARK-UDP  Huang et al., CVPR 2020: the same step on a 3 x 3 stencil with reflected borders (mmpose's post_dark_udp), and the W - 1 / H - 1 affine
// Argmax and score come from the RAW map in both, so the streaming pass above is all the map-sized work there is; the blurred, logged map is needed at the
// (2R + 1)^2 points around the argmax only (R = 2 for DARK, 1 for DARK-UDP), each a K x K window of raw values that the pass has just streamed (L2-hot).
// MAPPING.  The same one wavefront per map.  Behind wave_first every lane knows the argmax, and the whole wave evaluates the stencil, in wave-uniform control
// flow that does not depend on the map (an argmax on the border, a false mask: evaluated all the same, and not used), before lanes 1 .. 63 leave:
//   1 the horizontal sums h(row, col), col one of the 2R + 1 stencil columns, row one of the K + 2R rows the stencil's vertical sums touch: (2R + 1)(K + 2R) <= 105
//     ordered K-tap sums, one per lane, in up to two rounds of 64 (sum i sits in lane i & 63 of round i >> 6);
//   2 lane p < (2R + 1)^2 owns stencil point (p / (2R + 1) - R, p % (2R + 1) - R): its vertical sum takes the K horizontal sums it needs through __shfl, in
//     ascending order, then the clamp and the logarithm in fp64 (25 or 9 lanes at once; the step uses 13 or 7 of them);
//   3 13 or 7 fp64 shuffles hand those to lane 0, which makes the step, applies the affine and stores.
// No LDS, no second pass, no extra launch; the weights travel by value in the kernel arguments.  The streaming loops are the existing kernels' loops, restated as
// functions: moving the existing kernels themselves onto these functions changed their generated code (compare signedness, operand order), so they keep theirs.
constexpr int DM_QUARTER = 0, DM_DARK = 1, DM_UDP = 2;          // KASF_DECODE_*

struct Blur {                                                   // the separable Gaussian: K odd, 1 .. 17, weights w[0 .. K - 1] (the rest 0)
    float w[17];
    int K;
};

// one lane's share of one map, streamed: its first pair under comes_first (k_heatmap_keypoints' loop)
template <class E, bool VEC>
__device__ inline Best stream_map(const typename Elem<E>::T* __restrict__ map, int HW, int lane) {
    using T = typename Elem<E>::T;
    constexpr int VW = Elem<E>::VW;
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
    return {bv, bi};
}

// one lane's share of one merged map, streamed (and stored when mo is given): its first pair under comes_first (k_heatmap_flip_keypoints' loop)
template <class E, int MODE>
__device__ inline Best stream_merged(const typename Elem<E>::T* __restrict__ map, const typename Elem<E>::T* __restrict__ fmap, float* __restrict__ mo, int HW,
                                     int W, int shift, int lane) {
    using T = typename Elem<E>::T;
    constexpr int VW = Elem<E>::VW;
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
    return {bv, bi};
}

// reflect-101 of any index onto 0 .. n - 1: -i -> i, n - 1 + i -> n - 1 - i, with period 2 (n - 1); n = 1 always reads index 0
__device__ inline int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// kasf.h's L(v): the natural logarithm in fp64 by the library's own routine (argument reduction to [sqrt(1/2), sqrt(2)), the atanh series to z^11 in s = (m - 1) /
// (m + 1)), so that the device and a numpy restatement agree bit for bit; +inf and NaN come back as they are.  v is positive (clamped by the caller) or NaN.
__device__ inline double log_own(double v) {
    if (!(v < (double)INFINITY)) return v;
    int e;
    double m = frexp(v, &e);
    if (m < 0.7071067811865476) { m = 2.0 * m; e = e - 1; }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 23.0;
#pragma unroll
    for (int d = 21; d >= 1; d -= 2) p = p * z + 1.0 / (double)d;
    return (double)e * 0.6931471805599453 + 2.0 * s * p;
}

// The blurred, clamped, logged map at the stencil points around (py, px), by the whole wave: lane p < (2R + 1)^2 returns g(p / (2R + 1) - R, p % (2R + 1) - R),
// the other lanes a value nobody reads.  at(row, col) as finish takes it.  Every collective below is reached by all 64 lanes, the same number of times for
// every map of a launch.
template <class At>
__device__ inline double stencil_logs(int py, int px, int H, int W, int mode, const Blur& bl, int lane, At at) {
    const int K = bl.K, r = K / 2;
    const int R = mode == DM_DARK ? 2 : 1, NC = 2 * R + 1, NR = K + 2 * R, NH = NC * NR;      // NH <= 5 * 21
    // 1: horizontal sums, fp32, taps in ascending order, each product rounded and then added
    float h[2] = {0.0f, 0.0f};
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const int i = round * 64 + lane;
        if (i < NH) {
            const int c = i / NR, t = i - c * NR;
            const int yy = py - R - r + t, x0 = px - R + c - r;
            float acc = 0.0f;
            if (mode == DM_DARK) {                              // zero outside the map
                const bool row_in = 0 <= yy && yy < H;
                const int row = row_in ? yy * W : 0;
                for (int kh = 0; kh < K; ++kh) {
                    const int xx = x0 + kh;
                    const float v = row_in && 0 <= xx && xx < W ? at(row, xx) : 0.0f;
                    acc = acc + bl.w[kh] * v;
                }
            } else {                                            // reflect-101
                const int row = reflect101(yy, H) * W;
                for (int kh = 0; kh < K; ++kh) acc = acc + bl.w[kh] * at(row, reflect101(x0 + kh, W));
            }
            h[round] = acc;
        }
    }
    // 2: vertical sums, the same way, then the clamp and the logarithm
    const int p = lane < NC * NC ? lane : 0;
    int y = py + p / NC - R, x = px + p % NC - R;
    if (mode == DM_UDP) {                                       // mmpose's edge padding of the blurred map
        y = min(max(y, 0), H - 1);
        x = min(max(x, 0), W - 1);
    }
    const int first = (x - (px - R)) * NR + (y - (py - R));     // this point's topmost horizontal sum
    float acc = 0.0f;
    for (int kv = 0; kv < K; ++kv) {
        const int i = first + kv;
        float v = __shfl(h[0], i & 63);
        if (NH > 64) {
            const float v1 = __shfl(h[1], i & 63);
            v = i >= 64 ? v1 : v;
        }
        acc = acc + bl.w[kv] * v;
    }
    double b = (double)acc;
    if (mode == DM_DARK) {
        b = b < 1e-10 ? 1e-10 : b;
    } else {
        b = b < 0.001 ? 0.001 : b;
        b = b > 50.0 ? 50.0 : b;
    }
    return log_own(b);
}

// finish for kasf_heatmap_decode, reached by the whole wave: the stencil (modes 1, 2) by all lanes, then lane 0 alone -- the step, the affine, the store.
template <class At>
__device__ inline void finish_decode(float bv, int bi, int lane, int64_t m, int64_t person, int H, int W, const float* geom, int geom_kind, double aspect,
                                     int mode, const Blur& bl, int udp, float* out, At at) {
    int px = bi % W, py = bi / W;
    const bool found = bv > 0.0f;                               // get_max_preds' mask, false for a NaN
    if (!found) px = py = 0;
    double x = (double)px, y = (double)py;
    if (mode == DM_QUARTER) {
        if (lane != 0) return;
        if (1 < px && px < W - 1 && 1 < py && py < H - 1) {     // finish's POST_PROCESS
            const int row = py * W;
            x = (double)((float)px + sign_of(at(row, px + 1) - at(row, px - 1)) * 0.25f);
            y = (double)((float)py + sign_of(at(row + W, px) - at(row - W, px)) * 0.25f);
        }
    } else {
        const double g = stencil_logs(py, px, H, W, mode, bl, lane, at);
        const int R = mode == DM_DARK ? 2 : 1, NC = 2 * R + 1;
        auto G = [&](int dy, int dx) { return __shfl(g, (dy + R) * NC + dx + R); };
        const double g00 = G(0, 0), g0p = G(0, 1), g0m = G(0, -1), gp0 = G(1, 0), gm0 = G(-1, 0), gpp = G(1, 1), gmm = G(-1, -1);
        double a, b, d;
        if (mode == DM_DARK) {
            const double g0pp = G(0, 2), g0mm = G(0, -2), gpp0 = G(2, 0), gmm0 = G(-2, 0), gmp = G(-1, 1), gpm = G(1, -1);
            a = 0.25 * (g0pp - 2.0 * g00 + g0mm);
            d = 0.25 * (gpp0 - 2.0 * g00 + gmm0);
            b = 0.25 * (gpp - gmp - gpm + gmm);
        } else {
            const double eps = 1.1920928955078125e-07;          // 2^-23
            a = g0p - 2.0 * g00 + g0m + eps;
            d = gp0 - 2.0 * g00 + gm0 + eps;
            b = 0.5 * (gpp - g0p - gp0 + g00 + g00 - g0m - gm0 + gmm);
        }
        if (lane != 0) return;
        const bool step = found && (mode == DM_UDP || (1 < px && px < W - 2 && 1 < py && py < H - 2));
        const double gx = 0.5 * (g0p - g0m), gy = 0.5 * (gp0 - gm0);
        const double det = a * d - b * b;
        if (step && !(mode == DM_DARK && det == 0.0)) {         // nothing bounds the step; infinities and NaNs propagate
            x = (double)px - (d * gx - b * gy) / det;
            y = (double)py - (a * gy - b * gx) / det;
        }
    }
    const KasfCropGeom cg = kasf_crop_geom(geom + person * 4, geom_kind, aspect, W);
    float* o = out + m * 3;
    if (udp) {                                                  // UDP: W - 1 and H - 1 intervals, each axis by its own scale (H, W >= 2: the entry point)
        const float sw = cg.sx * 200.0f, sh = cg.sy * 200.0f;
        o[0] = (float)((double)cg.cx + (x - (double)(W - 1) * 0.5) * ((double)sw / (double)(W - 1)));
        o[1] = (float)((double)cg.cy + (y - (double)(H - 1) * 0.5) * ((double)sh / (double)(H - 1)));
    } else {                                                    // finish's affine
        o[0] = (float)((double)cg.cx + (x - (double)W * 0.5) * cg.kx);
        o[1] = (float)((double)cg.cy + (y - (double)H * 0.5) * cg.ky);
    }
    o[2] = bv;
}

template <class E, bool VEC>
__global__ __launch_bounds__(HM_THREADS) void k_heatmap_decode(const typename Elem<E>::T* __restrict__ hm, int64_t maps, int H, int W,
                                                               const float* __restrict__ geom, int geom_kind, double aspect, int mode, Blur bl, int udp,
                                                               float* __restrict__ out) {
    using T = typename Elem<E>::T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HW = H * W;                                       // <= 2^24 (checked by the entry point)
    for (int64_t m = (int64_t)blockIdx.x * HM_WAVES + wave; m < maps; m += (int64_t)gridDim.x * HM_WAVES) {   // the tail: a wave without a map leaves
        const T* __restrict__ map = hm + m * HW;
        const Best mine = stream_map<E, VEC>(map, HW, lane);
        const Best b = wave_first(mine.v, mine.i);
        finish_decode(b.v, b.i, lane, m, m / 17, H, W, geom, geom_kind, aspect, mode, bl, udp, out,
                      [&](int row, int col) { return Elem<E>::up(map[row + col]); });
    }
}

template <class E, int MODE>
__global__ __launch_bounds__(HM_THREADS) void k_heatmap_flip_decode(const typename Elem<E>::T* __restrict__ hm, const typename Elem<E>::T* __restrict__ hmf,
                                                                    int64_t maps, int H, int W, Partner partner, int shift, const float* __restrict__ geom,
                                                                    int geom_kind, double aspect, int mode, Blur bl, int udp, float* __restrict__ out,
                                                                    float* __restrict__ merged_out) {
    using T = typename Elem<E>::T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int HW = H * W;                                       // <= 2^24 (checked by the entry point)
    for (int64_t m = (int64_t)blockIdx.x * HM_WAVES + wave; m < maps; m += (int64_t)gridDim.x * HM_WAVES) {   // the tail: a wave without a map leaves
        const int64_t person = m / 17;
        const T* __restrict__ map = hm + m * HW;
        const T* __restrict__ fmap = hmf + (person * 17 + partner_of(partner, (int)(m - person * 17))) * HW;
        float* __restrict__ mo = merged_out ? merged_out + m * HW : nullptr;
        const Best mine = stream_merged<E, MODE>(map, fmap, mo, HW, W, shift, lane);
        const Best b = wave_first(mine.v, mine.i);
        // raw = the MERGED value, formed again from the two operands (never read back from merged_out)
        finish_decode(b.v, b.i, lane, m, person, H, W, geom, geom_kind, aspect, mode, bl, udp, out,
                      [&](int row, int col) { return merge(Elem<E>::up(map[row + col]), Elem<E>::up(fmap[row + src_x(col, W, shift)])); });
    }
}

Partner pack_partner(const int* partner) {
    Partner p = {0, 0};
    for (int j = 0; j < 17; ++j) {
        if (j < 12) p.lo |= (unsigned long long)(partner[j] & 31) << (5 * j);
        else p.hi |= (unsigned long long)(partner[j] & 31) << (5 * (j - 12));
    }
    return p;
}

template <class E>
void launch_decode(hipStream_t s, const void* hm, const void* hmf, int64_t maps, int H, int W, const int* partner, int shift, const float* geom, int geom_kind,
                   double aspect, int mode, const Blur& bl, int udp, float* out, float* merged_out) {
    using T = typename Elem<E>::T;
    const int64_t map_bytes = (int64_t)H * W * (int64_t)sizeof(T);
    const dim3 grid = hm_grid(maps), block(HM_THREADS);
    const T* a = (const T*)hm;
    const T* b = (const T*)hmf;
    if (!hmf) {
        const bool vec = ((uintptr_t)hm & 15) == 0 && (map_bytes & 15) == 0;
        if (vec) hipLaunchKernelGGL((k_heatmap_decode<E, true>), grid, block, 0, s, a, maps, H, W, geom, geom_kind, aspect, mode, bl, udp, out);
        else hipLaunchKernelGGL((k_heatmap_decode<E, false>), grid, block, 0, s, a, maps, H, W, geom, geom_kind, aspect, mode, bl, udp, out);
        return;
    }
    const Partner p = pack_partner(partner);
    const bool vec = (((uintptr_t)hm | (uintptr_t)hmf | (uintptr_t)merged_out) & 15) == 0 && (map_bytes & 15) == 0;
    const int path = !vec ? ELEM : (W % Elem<E>::VW == 0 ? ROW : SPLIT);
    if (path == ROW)
        hipLaunchKernelGGL((k_heatmap_flip_decode<E, ROW>), grid, block, 0, s, a, b, maps, H, W, p, shift, geom, geom_kind, aspect, mode, bl, udp, out, merged_out);
    else if (path == SPLIT)
        hipLaunchKernelGGL((k_heatmap_flip_decode<E, SPLIT>), grid, block, 0, s, a, b, maps, H, W, p, shift, geom, geom_kind, aspect, mode, bl, udp, out, merged_out);
    else
        hipLaunchKernelGGL((k_heatmap_flip_decode<E, ELEM>), grid, block, 0, s, a, b, maps, H, W, p, shift, geom, geom_kind, aspect, mode, bl, udp, out, merged_out);
}

}  // namespace

void kasf_launch_heatmap_decode(hipStream_t s, const void* hm, const void* hmf, int dtype, int64_t n, int H, int W, const int* partner, int shift,
                                const float* geom, int geom_kind, double aspect, int mode, const float* weights, int K, int udp, float* out, float* merged_out) {
    if (n <= 0) return;
    Blur bl;
    for (int k = 0; k < 17; ++k) bl.w[k] = mode != DM_QUARTER && k < K ? weights[k] : 0.0f;
    bl.K = K;
    if (dtype == KASF_F32) launch_decode<F32>(s, hm, hmf, n * 17, H, W, partner, shift, geom, geom_kind, aspect, mode, bl, udp, out, merged_out);
    else if (dtype == KASF_F16) launch_decode<F16>(s, hm, hmf, n * 17, H, W, partner, shift, geom, geom_kind, aspect, mode, bl, udp, out, merged_out);
    else launch_decode<BF16>(s, hm, hmf, n * 17, H, W, partner, shift, geom, geom_kind, aspect, mode, bl, udp, out, merged_out);
}

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
