// Host stand-in for csrc/kernels.h, for tests/test_track_host_cpu.py only: just what csrc/k_track.hip needs to compile with g++, and a lockstep emulation of one
// wave64 workgroup -- 64 host threads, a barrier at every collective (__shfl, __shfl_xor, __ballot, __syncthreads).  That is a faithful model exactly when every
// collective sits in wave-uniform control flow, which the kernel is written to guarantee; a collective in divergent control flow deadlocks here (the test's
// time limit reports it) instead of returning garbage.  __shared__ becomes a function-level static: one workgroup runs at a time.
#pragma once
#include <cstdint>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <thread>
#include <vector>
#include <barrier>
#define KASF_SORT_HEADER_BYTES 64
#define __global__
#define __device__
#define __shared__ static
#define __launch_bounds__(x)
typedef void* hipStream_t;
struct dim3 { int x; dim3(int a) : x(a) {} };
struct Idx { int x; };
extern thread_local Idx threadIdx, blockIdx;
using std::min; using std::max;
extern std::barrier<>* g_bar;
extern unsigned long long g_slot64[64];
inline void __syncthreads() { g_bar->arrive_and_wait(); }
template <class T> inline T xchg(T v, int src) {
    static_assert(sizeof(T) <= 8, "");
    unsigned long long raw = 0; memcpy(&raw, &v, sizeof(T));
    g_slot64[threadIdx.x] = raw;
    g_bar->arrive_and_wait();
    unsigned long long got = g_slot64[src & 63];
    g_bar->arrive_and_wait();
    T out; memcpy(&out, &got, sizeof(T)); return out;
}
template <class T> inline T __shfl(T v, int src) { return xchg(v, src); }
template <class T> inline T __shfl_xor(T v, int off) { return xchg(v, threadIdx.x ^ off); }
inline unsigned long long __ballot(bool p) {
    g_slot64[threadIdx.x] = p ? 1 : 0;
    g_bar->arrive_and_wait();
    unsigned long long m = 0;
    for (int i = 0; i < 64; ++i) m |= (g_slot64[i] & 1ull) << i;
    g_bar->arrive_and_wait();
    return m;
}
inline int __popcll(unsigned long long m) { return __builtin_popcountll(m); }
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, arg) emul_launch([=]() { kern(arg); }, (grid).x)
template <class F> void emul_launch(F f, int nblocks) {
    for (int b = 0; b < nblocks; ++b) {
        std::barrier<> bar(64);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (int l = 0; l < 64; ++l) th.emplace_back([=]() { threadIdx.x = l; blockIdx.x = b; f(); });
        for (auto& t : th) t.join();
    }
}
