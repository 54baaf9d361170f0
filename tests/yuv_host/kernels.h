// Host stand-in for csrc/kernels.h, for tests/test_yuv_host_cpu.py only: just what csrc/k_yuv.hip needs to compile with g++, and a lockstep emulation of its
// workgroups -- one host thread per GPU thread of a block, the blocks of the two-dimensional grid one after the other, a barrier at every __syncthreads (the
// kernel has none today; one added later is modelled), no LDS: a launch that asks for dynamic LDS is counted as an error.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include <barrier>
#define __global__
#define __device__
#define __launch_bounds__(x)
typedef void* hipStream_t;
struct dim3 { unsigned x, y; dim3(unsigned a, unsigned b = 1) : x(a), y(b) {} };
struct Idx { unsigned x, y; };
extern thread_local Idx threadIdx, blockIdx, gridDim;
extern std::barrier<>* g_bar;
extern int g_lds_asked, g_launches;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline int __mul24(int a, int b) { return (int)((unsigned)a << 8) / 256 * ((int)((unsigned)b << 8) / 256); }      // the low 24 bits of each operand, sign-extended

template <class F> void emul_launch(F f, dim3 grid, unsigned nthreads, size_t lds_bytes) {
    g_lds_asked |= lds_bytes != 0;
    ++g_launches;
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::barrier<> bar(nthreads);
            g_bar = &bar;
            std::vector<std::thread> th;
            for (unsigned l = 0; l < nthreads; ++l)
                th.emplace_back([=]() { threadIdx = Idx{l, 0}; blockIdx = Idx{bx, by}; gridDim = Idx{grid.x, grid.y}; f(); });
            for (auto& t : th) t.join();
        }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) emul_launch([=]() { kern(__VA_ARGS__); }, (grid), (block).x, (lds))
