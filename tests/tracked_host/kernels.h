// Host stand-in for csrc/kernels.h, for tests/test_tracked_host_cpu.py and tests/test_lift_host_cpu.py only: just what csrc/k_stream_track.hip and csrc/k_lift.hip
// need to compile with g++, and a lockstep emulation of their workgroups -- one host thread per GPU thread of a block, the blocks one after the other, a barrier at every __syncthreads / __syncthreads_or.  That is a
// faithful model exactly when every barrier sits in block-uniform control flow, which the kernels are written to guarantee; a barrier in divergent control flow
// deadlocks here (the test's time limit reports it) instead of returning garbage.
#pragma once
#include <cstdint>
#include <cstring>
#include <atomic>
#include <thread>
#include <vector>
#include <barrier>
#define KASF_ROWS_PERSONS 0
#define KASF_ROWS_TRACKS 1
#define __global__
#define __device__
#define __constant__ static const
#define __launch_bounds__(x)
typedef void* hipStream_t;
struct dim3 { unsigned x; dim3(unsigned a) : x(a) {} };
struct Idx { unsigned x; };
extern thread_local Idx threadIdx, blockIdx, gridDim;
struct alignas(16) float4 { float x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
extern std::barrier<>* g_bar;
extern std::atomic<int> g_or[2];
extern thread_local int g_phase;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline int __syncthreads_or(int p) {
    std::atomic<int>& acc = g_or[g_phase & 1];
    if (p) acc.store(1);
    g_bar->arrive_and_wait();
    const int got = acc.load();
    g_or[(g_phase + 1) & 1].store(0);                  // the other cell is idle until the next call, which every thread reaches after the barrier below
    g_bar->arrive_and_wait();
    ++g_phase;
    return got;
}
template <class F> void emul_launch(F f, unsigned nblocks, unsigned nthreads) {
    for (unsigned b = 0; b < nblocks; ++b) {
        std::barrier<> bar(nthreads);
        g_bar = &bar;
        g_or[0].store(0);
        g_or[1].store(0);
        std::vector<std::thread> th;
        for (unsigned l = 0; l < nthreads; ++l) th.emplace_back([=]() { threadIdx.x = l; blockIdx.x = b; gridDim.x = nblocks; g_phase = 0; f(); });
        for (auto& t : th) t.join();
    }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) emul_launch([=]() { kern(__VA_ARGS__); }, (grid).x, (block).x)
#include "lift_math.h"                                 // the real one, copied next to the kernel source by the fixture
