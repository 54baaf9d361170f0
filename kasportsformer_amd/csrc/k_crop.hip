// Person boxes -> pose-network inputs (kasf.h, kasf_crop_persons): what the demo's PreProcess does on the host in front of HRNet
//   box_to_center_scale, get_affine_transform       demo/lib/hrnet/lib/utils/utilitys.py:102-169, transforms.py:58-101 (crop_geom.h, shared with k_heatmap.hip)
//   cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT)   restated as the 10-bit fixed-point positions / 5-bit fractions of OpenCV's portable path (kasf.h, rules 2-3)
//   ToTensor, Normalize, the [:, [2, 1, 0]] swap         rule 4: a 3 x 256 table of normalised outputs, planes stored swapped
// One launch, no atomics, no scratch, nothing that depends on n: a person's planes are a function of its own geom row and frame alone.
// MAPPING.  A workgroup of 256 threads serves one person (blockIdx.y, strided past 65,535) and walks chunks of 256 "groups"; a group is PX consecutive pixels
// of one output row, PX = 16 bytes of the output type (4 fp32, 8 fp16 / bf16), so each of a thread's three planes leaves in ONE 16-byte store and a wavefront's
// store instruction covers 1 KiB of consecutive addresses.  Crops whose width is not a multiple of PX, or whose base is not 16-byte aligned (33 x 31, 5 x 3),
// take the same kernel with PX = 1 (element stores, still consecutive across lanes).
// Per thread: Y0 once (its row), ad[x] once per pixel, then per pixel the four taps of three channels = 12 byte loads, unaligned by nature (3 bytes per
// frame pixel); neighbouring lanes read neighbouring or equal taps, and a 1080p frame (6 MB) stays in L2.  The bilinear sum is integer (an exact 0..255), and
// only 3 x 256 normalised outputs exist: they are formed once per workgroup, already rounded to the output type, in LDS (1.5 - 3 KiB) and indexed -- the two
// fp32 divisions of rule 4 are paid 768 times per workgroup, not per value.  Thread 0 derives the person's geometry (two fp64 divisions) while the others
// fill the table; one barrier publishes both.
#include "kernels.h"
#include "crop_geom.h"

namespace {

constexpr int CROP_THREADS = 256;

struct CropNorm { float mean[3], std[3]; };                    // per FRAME channel

struct PersonGeom {                                            // what thread 0 leaves in LDS for its workgroup
    double kx, ky, by;
    long long X0;
    int ok;                                                    // 0: the whole crop is border (non-finite geometry, or a frame index out of range)
    int frame;
};

template <class T> __device__ inline T to_out(float f);
template <> __device__ inline float to_out<float>(float f) { return f; }
template <> __device__ inline _Float16 to_out<_Float16>(float f) { return (_Float16)f; }      // round to nearest even
template <> __device__ inline __bf16 to_out<__bf16>(float f) { return (__bf16)f; }            // round to nearest even

__device__ inline bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }       // false for a NaN

// rule 2: rint (half to even), saturated at +-2^61 so that sums of two stay inside 64 bits
__device__ inline long long fix(double v) {
    const double lim = 2305843009213693952.0;
    return (long long)fmin(fmax(rint(v), -lim), lim);
}

template <class T, int PX>
__global__ __launch_bounds__(CROP_THREADS) void k_crop_persons(const unsigned char* __restrict__ frames, int n_frames, int Hf, int Wf, int64_t row_stride,
                                                              int64_t frame_stride, const int* __restrict__ frame_index, const float* __restrict__ geom,
                                                              int geom_kind, double aspect, int64_t n, T* __restrict__ out, int out_w, int out_h,
                                                              CropNorm nm, int swap_rb, float* __restrict__ cs_out) {
    __shared__ T table[3 * 256];
    __shared__ PersonGeom pg;
    const int tid = threadIdx.x;
    // rule 4, for every value a channel can take: two roundings of a division, one of a subtraction, then the output type's
    for (int e = tid; e < 3 * 256; e += CROP_THREADS) {
        const int c = e >> 8;
        table[e] = to_out<T>(((float)(e & 255) / 255.0f - nm.mean[c]) / nm.std[c]);
    }
    const int gpr = (out_w + PX - 1) / PX;                      // groups per row
    const int groups = gpr * out_h;                             // <= 2^30 (out_w, out_h <= 32,767)
    const int64_t plane = (int64_t)out_h * out_w;
    for (int64_t p = blockIdx.y; p < n; p += gridDim.y) {
        __syncthreads();                                        // the previous person's readers are done with pg
        if (tid == 0) {
            const KasfCropGeom cg = kasf_crop_geom(geom + p * 4, geom_kind, aspect, out_w);
            // rule 1: crop pixel (x, y) sits at frame position (bx + kx x, by + ky y)
            const double bx = (double)cg.cx - ((double)out_w * 0.5) * cg.kx;
            const double by = (double)cg.cy - ((double)out_h * 0.5) * cg.ky;
            const int fi = frame_index ? frame_index[p] : 0;
            pg.kx = cg.kx; pg.ky = cg.ky; pg.by = by;
            pg.X0 = fix(bx * 1024.0) + 16;
            pg.ok = finite_d(cg.kx) && finite_d(cg.ky) && finite_d(bx) && finite_d(by) && fi >= 0 && fi < n_frames;
            pg.frame = fi;
            if (cs_out && blockIdx.x == 0) {
                float* o = cs_out + p * 4;
                o[0] = cg.cx; o[1] = cg.cy; o[2] = cg.sx; o[3] = cg.sy;
            }
        }
        __syncthreads();                                        // also publishes the table
        const double kx = pg.kx, ky = pg.ky, by = pg.by;
        const long long X0 = pg.X0;
        const bool ok = pg.ok != 0;
        const unsigned char* __restrict__ frame = frames + (ok ? (int64_t)pg.frame * frame_stride : 0);
        T* __restrict__ op = out + p * 3 * plane;
        for (int g = blockIdx.x * CROP_THREADS + tid; g < groups; g += gridDim.x * CROP_THREADS) {
            const int y = g / gpr, x0 = (g - y * gpr) * PX;
            const long long Y = (fix((ky * (double)y + by) * 1024.0) + 16) >> 5;
            const long long ty = Y >> 5;
            const int fy = (int)(Y & 31);
            const bool r0 = ok && (unsigned long long)ty < (unsigned long long)Hf;
            const bool r1 = ok && (unsigned long long)(ty + 1) < (unsigned long long)Hf;
            const unsigned char* __restrict__ row0 = frame + (r0 ? ty * row_stride : 0);        // dereferenced only under r0 / r1
            const unsigned char* __restrict__ row1 = frame + (r1 ? (ty + 1) * row_stride : 0);
            T val[3][PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const long long X = (X0 + fix((kx * (double)(x0 + j)) * 1024.0)) >> 5;
                const long long tx = X >> 5;
                const int fx = (int)(X & 31);
                const bool c0 = (unsigned long long)tx < (unsigned long long)Wf;
                const bool c1 = (unsigned long long)(tx + 1) < (unsigned long long)Wf;
                const int64_t o0 = c0 ? tx * 3 : 0, o1 = c1 ? (tx + 1) * 3 : 0;                 // inside the row whenever they are read
                const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int p00 = (r0 && c0) ? row0[o0 + c] : 0;                            // rule 3: a tap outside the frame counts 0, each on its own
                    const int p01 = (r0 && c1) ? row0[o1 + c] : 0;
                    const int p10 = (r1 && c0) ? row1[o0 + c] : 0;
                    const int p11 = (r1 && c1) ? row1[o1 + c] : 0;
                    const int v = (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10;  // 0 .. 255
                    val[c][j] = table[c * 256 + v];
                }
            }
            T* __restrict__ o = op + (int64_t)y * out_w + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                T* __restrict__ dst = o + (swap_rb ? 2 - c : c) * plane;                      // rule 4: plane k holds frame channel 2 - k
                if (PX == 1) {
                    dst[0] = val[c][0];
                } else {
                    struct alignas(16) Vec { T e[PX]; };
                    Vec v;
#pragma unroll
                    for (int j = 0; j < PX; ++j) v.e[j] = val[c][j];
                    *reinterpret_cast<Vec*>(dst) = v;
                }
            }
        }
    }
}

template <class T>
void launch(hipStream_t s, const unsigned char* frames, int n_frames, int Hf, int Wf, int64_t row_stride, int64_t frame_stride, const int* frame_index,
            const float* geom, int geom_kind, double aspect, int64_t n, void* out, int out_w, int out_h, const CropNorm& nm, int swap_rb, float* cs_out) {
    constexpr int VPX = 16 / (int)sizeof(T);
    const bool vec = ((uintptr_t)out & 15) == 0 && out_w % VPX == 0;    // then every row of every plane starts on a 16-byte boundary
    const int px = vec ? VPX : 1;
    const int64_t groups = (int64_t)((out_w + px - 1) / px) * out_h;
    int64_t bpp = (groups + CROP_THREADS - 1) / CROP_THREADS;           // workgroups per person: one chunk each while that keeps the launch under ~8 per CU,
    if (n * bpp > 2048) bpp = (bpp + 3) / 4;                            // four chunks each beyond (the table is formed once per workgroup)
    const dim3 grid((unsigned)bpp, (unsigned)(n > 65535 ? 65535 : n)), block(CROP_THREADS);
    if (vec)
        hipLaunchKernelGGL((k_crop_persons<T, VPX>), grid, block, 0, s, frames, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, geom_kind, aspect,
                           n, (T*)out, out_w, out_h, nm, swap_rb, cs_out);
    else
        hipLaunchKernelGGL((k_crop_persons<T, 1>), grid, block, 0, s, frames, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, geom_kind, aspect,
                           n, (T*)out, out_w, out_h, nm, swap_rb, cs_out);
}

}  // namespace

void kasf_launch_crop_persons(hipStream_t s, const void* frames, int n_frames, int Hf, int Wf, int64_t row_stride, int64_t frame_stride,
                              const int* frame_index, const float* geom, int geom_kind, double aspect, int64_t n, void* out, int out_dtype, int out_w,
                              int out_h, const float* mean_std, int swap_rb, float* center_scale_out) {
    if (n <= 0) return;
    CropNorm nm;
    for (int c = 0; c < 3; ++c) { nm.mean[c] = mean_std[c]; nm.std[c] = mean_std[3 + c]; }
    const unsigned char* f = (const unsigned char*)frames;
    if (out_dtype == KASF_F32)
        launch<float>(s, f, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, geom_kind, aspect, n, out, out_w, out_h, nm, swap_rb, center_scale_out);
    else if (out_dtype == KASF_F16)
        launch<_Float16>(s, f, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, geom_kind, aspect, n, out, out_w, out_h, nm, swap_rb, center_scale_out);
    else
        launch<__bf16>(s, f, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, geom_kind, aspect, n, out, out_w, out_h, nm, swap_rb, center_scale_out);
}
