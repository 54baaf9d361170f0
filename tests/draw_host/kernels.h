// Host stand-in for csrc/kernels.h, for tests/test_draw_host_cpu.py only: just what csrc/k_draw.hip needs to compile with g++, and a lockstep emulation of its
// workgroups -- one host thread per GPU thread of a block, the blocks of the two-dimensional grid one after the other, a barrier at every __syncthreads.
// __shared__ arrays are statics (one block runs at a time); __ballot is modelled per wavefront of 64 consecutive threads: every thread of the block posts its
// predicate, a barrier, every thread reads its own wavefront's 64, a barrier -- which is right as long as every thread of the block reaches the same __ballot,
// as k_draw.hip's do (its ballots sit in block-uniform control flow).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include <barrier>
#include "draw_args.h"
#define __global__
#define __device__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(x)
typedef void* hipStream_t;
struct dim3 { unsigned x, y; dim3(unsigned a, unsigned b = 1) : x(a), y(b) {} };
struct Idx { unsigned x, y; };
extern thread_local Idx threadIdx, blockIdx, gridDim;
extern std::barrier<>* g_bar;
extern int g_launches;
extern unsigned char g_pred[1024];
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline unsigned long long __ballot(int pred) {
    g_pred[threadIdx.x] = pred != 0;
    g_bar->arrive_and_wait();
    unsigned long long m = 0;
    const unsigned w0 = threadIdx.x & ~63u;
    for (unsigned l = 0; l < 64; ++l) m |= (unsigned long long)g_pred[w0 + l] << l;
    g_bar->arrive_and_wait();
    return m;
}
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline float __fadd_rn(float a, float b) { return a + b; }       // compiled with -ffp-contract=off: one rounding each
inline float __fsub_rn(float a, float b) { return a - b; }
inline float __fmul_rn(float a, float b) { return a * b; }

template <class F> void emul_launch(F f, dim3 grid, unsigned nthreads) {
    ++g_launches;
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::memset(g_pred, 0, sizeof g_pred);
            std::barrier<> bar(nthreads);
            g_bar = &bar;
            std::vector<std::thread> th;
            for (unsigned l = 0; l < nthreads; ++l)
                th.emplace_back([=]() { threadIdx = Idx{l, 0}; blockIdx = Idx{bx, by}; gridDim = Idx{grid.x, grid.y}; f(); });
            for (auto& t : th) t.join();
        }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) emul_launch([=]() { kern(__VA_ARGS__); }, (grid), (block).x)
