// AdamW and the global gradient norm over a LIST of element ranges of the flat fp32 arrays (kasf_adamw_segments, kasf_grad_norm): what a torch.optim-shaped
// optimiser needs on top of k_adamw's one range [0, n) -- parameter groups with their own hyper-parameters, frozen or gradient-less parameters in between, a
// step count per parameter, clipping by the norm of exactly the parameters that step.
//
// Both kernels walk a chunk table (KasfOptChunk, include/kasf.h; built by the host, kasportsformer_amd/optim.py: plan_chunks): a chunk is at most
// KASF_OPT_CHUNK_MAX consecutive elements of one class, `begin` and `count` arbitrary.  A workgroup takes one chunk at a time, grid-stride over chunks; within a
// chunk the elements up to the first 16-byte boundary and behind the last one go through scalar accesses, the middle as f32x4 like k_adamw.  Nothing outside
// the listed elements is read-modified or written.
//
//   k_adamw_seg         the update.  The classes -- {lr, beta1, beta2, eps, weight_decay, bc1, bc2} each -- travel by value in the kernel arguments, so a
//                       learning-rate change costs no upload.  Per element the statements are k_adamw's (k_misc.hip), `gs` replaced by
//                       s = clip ? grad_scale * clip[1] : grad_scale: one class and one aligned run [0, n) without clip give kasf_adamw_step's bits.
//   k_grad_sumsq        one double per chunk: the sum of (double)g * (double)g in an order fixed by the chunk's (begin, count) alone -- a thread's own elements
//                       in ascending order, the xor butterfly over a wave, the four waves as (0 + 1) + (2 + 3).  Stored, never added atomically.
//   k_grad_norm_finish  one workgroup: thread t adds partials t, t + 256, ... in index order, a fixed tree over the 256 threads, then
//                       norm = (float)(sqrt(total) * grad_scale) and coef = min(1, max_norm / (norm + 1e-6f)) with torch's NaN propagation.
// Pure streaming: 16 B read + 12 B written per element and 16 B of table per chunk for the update, 4 B read per element for the norm.
#include "kernels.h"
#include "kasf.h"      // KasfOptChunk, KasfAdamwClasses

namespace {

typedef float f32x4 __attribute__((vector_size(16)));      // common.h's type under g++'s spelling: this file also compiles for the host (tests/host_emul)

// k_adamw's statements for one element (k_misc.hip), `gs` being `s` here
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd, float step, float isq,
                                              float s) {
    const float gr = g * s;
    p *= 1.0f - lr * wd;
    m = b1 * m + (1.0f - b1) * gr;
    v = b2 * v + (1.0f - b2) * gr * gr;
    p -= step * m / (sqrtf(v) * isq + eps);
}

// a chunk [begin, begin + count) of arrays whose bases are 16-byte aligned: `head` elements up to the first aligned one, n4 whole f32x4, `tail` elements behind
struct ChunkSplit {
    int64_t mid;       // element index of the first f32x4
    int head, n4, tail;
};
__device__ __forceinline__ ChunkSplit split_chunk(int64_t begin, int count) {
    ChunkSplit c;
    c.head = (int)((4 - (begin & 3)) & 3);
    if (c.head > count) c.head = count;
    c.n4 = (count - c.head) >> 2;
    c.tail = count - c.head - 4 * c.n4;
    c.mid = begin + c.head;
    return c;
}

__global__ __launch_bounds__(256) void k_adamw_seg(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   const KasfOptChunk* __restrict__ chunks, int64_t n_chunks, KasfAdamwClasses cls, float grad_scale,
                                                   const float* __restrict__ clip) {
    const float s = clip != nullptr ? grad_scale * clip[1] : grad_scale;
    const int t = (int)threadIdx.x;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const KasfOptChunk ch = chunks[c];
        const KasfAdamwClass k = cls.c[ch.cls & (KASF_OPT_MAX_CLASSES - 1)];
        const float lr = k.lr, b1 = k.beta1, b2 = k.beta2, eps = k.eps, wd = k.weight_decay;
        const float step = lr / k.bc1, isq = 1.0f / sqrtf(k.bc2);
        const ChunkSplit sp = split_chunk(ch.begin, ch.count);
        if (t < sp.head) {
            const int64_t i = ch.begin + t;
            adamw_element(p[i], g[i], m[i], v[i], lr, b1, b2, eps, wd, step, isq, s);
        }
        const int64_t q0 = sp.mid >> 2;
        for (int j = t; j < sp.n4; j += 256) {
            const int64_t i = q0 + j;
            f32x4 pp = reinterpret_cast<f32x4*>(p)[i], gg = reinterpret_cast<const f32x4*>(g)[i], mm = reinterpret_cast<f32x4*>(m)[i],
                  vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pp[e], me = mm[e], ve = vv[e];
                adamw_element(pe, gg[e], me, ve, lr, b1, b2, eps, wd, step, isq, s);
                pp[e] = pe; mm[e] = me; vv[e] = ve;
            }
            reinterpret_cast<f32x4*>(p)[i] = pp;
            reinterpret_cast<f32x4*>(m)[i] = mm;
            reinterpret_cast<f32x4*>(v)[i] = vv;
        }
        if (t < sp.tail) {
            const int64_t i = sp.mid + 4 * (int64_t)sp.n4 + t;
            adamw_element(p[i], g[i], m[i], v[i], lr, b1, b2, eps, wd, step, isq, s);
        }
    }
}

__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, const KasfOptChunk* __restrict__ chunks, int64_t n_chunks,
                                                    double* __restrict__ partial) {
    __shared__ double sW[2][4];      // the four waves' sums, two sets: chunk k + 1 writes the other one while thread 0 may still read chunk k's
    const int t = (int)threadIdx.x;
    int flip = 0;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x, flip ^= 1) {
        const KasfOptChunk ch = chunks[c];
        const ChunkSplit sp = split_chunk(ch.begin, ch.count);
        double a = 0.0;
        if (t < sp.head) { const double x = (double)g[ch.begin + t]; a += x * x; }
        const int64_t q0 = sp.mid >> 2;
        for (int j = t; j < sp.n4; j += 256) {
            const f32x4 gg = reinterpret_cast<const f32x4*>(g)[q0 + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double x = (double)gg[e]; a += x * x; }
        }
        if (t < sp.tail) { const double x = (double)g[sp.mid + 4 * (int64_t)sp.n4 + t]; a += x * x; }
        for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off);
        if ((t & 63) == 0) sW[flip][t >> 6] = a;
        __syncthreads();
        if (t == 0) partial[c] = (sW[flip][0] + sW[flip][1]) + (sW[flip][2] + sW[flip][3]);
    }
}

__global__ __launch_bounds__(256) void k_grad_norm_finish(const double* __restrict__ partial, int64_t n_chunks, float grad_scale, float max_norm,
                                                          float* __restrict__ out2) {
    __shared__ double sP[256];
    const int t = (int)threadIdx.x;
    double a = 0.0;
    for (int64_t i = t; i < n_chunks; i += 256) a += partial[i];
    sP[t] = a;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (t < h) sP[t] += sP[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const float norm = (float)(sqrt(sP[0]) * (double)grad_scale);
        const float q = max_norm / (norm + 1e-6f);
        out2[0] = norm;
        out2[1] = q > 1.0f ? 1.0f : q;      // torch.clamp(q, max=1.0): a NaN stays a NaN
    }
}

// one workgroup per chunk up to the cap, as ew_grid caps k_adamw's grid (8 workgroups of 256 per CU)
inline unsigned chunk_grid(int64_t n_chunks, int cap) { return (unsigned)(n_chunks > cap ? cap : (n_chunks < 1 ? 1 : n_chunks)); }

}  // namespace

void kasf_launch_adamw_segments(hipStream_t s, float* p, const float* g, float* m, float* v, const KasfOptChunk* chunks, int64_t n_chunks,
                                const KasfAdamwClasses& classes, float grad_scale, const float* clip, int grid_cap) {
    if (n_chunks < 1) return;
    hipLaunchKernelGGL(k_adamw_seg, dim3(chunk_grid(n_chunks, grid_cap)), dim3(256), 0, s, p, g, m, v, chunks, n_chunks, classes, grad_scale, clip);
}
void kasf_launch_grad_norm(hipStream_t s, const float* g, const KasfOptChunk* chunks, int64_t n_chunks, double* partial, float grad_scale, float max_norm,
                           float* out2, int grid_cap) {
    if (n_chunks < 1) return;
    hipLaunchKernelGGL(k_grad_sumsq, dim3(chunk_grid(n_chunks, grid_cap)), dim3(256), 0, s, g, chunks, n_chunks, partial);
    hipLaunchKernelGGL(k_grad_norm_finish, dim3(1), dim3(256), 0, s, (const double*)partial, n_chunks, grad_scale, max_norm, out2);
}
