// Host stand-in for csrc/kernels.h, for tests/test_loss_host_cpu.py only: just what csrc/k_loss.hip (and the k_loss3 text of csrc/k_misc.hip) needs to compile
// with g++, and a lockstep emulation of a workgroup -- one host thread per GPU thread of a block, the blocks one after the other, a barrier at every
// __syncthreads.  __shared__ arrays are statics (one block runs at a time), the dynamic LDS is one array of the launch's size.  __shfl_xor is modelled per
// wavefront of 64 consecutive threads: every thread of the block posts its value, a barrier, every thread reads its partner's inside its own wavefront, a
// barrier -- which is right as long as every thread of the block reaches the same shuffle, as the loss kernels' do (their reductions sit in block-uniform
// control flow).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include <barrier>
#define __global__
#define __device__
#define __constant__
#define __forceinline__ inline
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
typedef void* hipStream_t;
struct dim3 { unsigned x; dim3(unsigned a) : x(a) {} };
struct Idx { unsigned x; };
extern thread_local Idx threadIdx, blockIdx;
extern std::barrier<>* g_bar;
extern int g_launches;
extern float g_slot[1024];
extern float* g_dyn_lds;
#define KASF_DYNAMIC_LDS(name) float* name = g_dyn_lds
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline float __shfl_xor(float v, int off) {
    g_slot[threadIdx.x] = v;
    g_bar->arrive_and_wait();
    const float got = g_slot[(threadIdx.x & ~63u) | ((threadIdx.x ^ (unsigned)off) & 63u)];
    g_bar->arrive_and_wait();
    return got;
}
template <class F> void emul_launch(F f, dim3 grid, unsigned nthreads, size_t lds_bytes) {
    ++g_launches;
    std::vector<float> lds((lds_bytes + sizeof(float) - 1) / sizeof(float));       // to the word: an overrun is the sanitizer build's to find
    g_dyn_lds = lds.data();
    for (unsigned bx = 0; bx < grid.x; ++bx) {
        std::barrier<> bar(nthreads);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (unsigned l = 0; l < nthreads; ++l) th.emplace_back([=]() { threadIdx = Idx{l}; blockIdx = Idx{bx}; f(); });
        for (auto& t : th) t.join();
    }
    g_dyn_lds = nullptr;
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) emul_launch([=]() { kern(__VA_ARGS__); }, (grid), (block).x, (lds))
void kasf_launch_loss7(hipStream_t s, const float* pred, const float* tgt, float* dpred, float* losses, int B, int T, const float* lambdas, float grad_scale);
void kasf_launch_loss3(hipStream_t s, const float* pred, const float* tgt, float* dpred, float* losses, int B, int T, float lambda_n, float lambda_v,
                       float grad_scale);
