// Host stand-in for <hip/hip_runtime.h>, first on the include path of the host-compiled kernel tests (tests/host_emul/__init__.py): a kernel's own source and
// the real csrc/kernels.h compile with g++ behind it, and a launch runs as a lockstep emulation of its workgroups -- one host thread per GPU thread of a block,
// the blocks of the grid one after the other, a barrier at every __syncthreads and two around every wave collective.  The model is faithful exactly when every
// barrier sits in block-uniform control flow and every collective in wave-uniform control flow that all waves of the block reach alike; a divergent one
// deadlocks here (the test's time limit reports it) instead of returning garbage.  tests/test_host_emul_cpu.py tests this file on its own.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

// ---- qualifiers and basic types (__restrict__ is g++'s own keyword, honoured as hipcc honours it) ----
#define __global__
#define __device__
#define __host__
#define __constant__ static
#define __forceinline__ inline
#define __shared__ static                              // one block runs at a time
#define __launch_bounds__(...)
typedef void* hipStream_t;
struct dim3 {
    unsigned x, y, z;
    constexpr dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
inline thread_local dim3 threadIdx, blockIdx, gridDim, blockDim;
struct alignas(16) float4 { float x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
using std::max;
using std::min;
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __mul24(int a, int b) { return (int)((unsigned)a << 8) / 256 * ((int)((unsigned)b << 8) / 256); }      // the low 24 bits of each operand, sign-extended
inline float __fadd_rn(float a, float b) { return a + b; }       // compiled with -ffp-contract=off: one rounding each
inline float __fsub_rn(float a, float b) { return a - b; }
inline float __fmul_rn(float a, float b) { return a * b; }

// ---- the 16-bit types: two small classes that round a float to nearest even in software (this g++ may have neither _Float16 nor __bf16); every standard
// header is included BEFORE their names are defined as macros ----
struct emu_half {                                      // IEEE binary16 from a float
    uint16_t bits;
    emu_half() = default;
    explicit emu_half(float f) {
        uint32_t x;
        std::memcpy(&x, &f, 4);
        const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
        x &= 0x7fffffffu;
        if (x >= 0x7f800000u) { bits = sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u); return; }
        if (x < 0x38800000u) { bits = sign | (uint16_t)std::nearbyint(std::fabs(f) * 16777216.0f); return; }       // below 2^-14: a multiple of 2^-24
        uint32_t h = (((x >> 23) - 112u) << 10) | ((x & 0x7fffffu) >> 13);
        const uint32_t rem = x & 0x1fffu;
        if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;                                                      // a carry runs into the exponent
        bits = sign | (uint16_t)(h > 0x7c00u ? 0x7c00u : h);
    }
};
struct emu_bf16 {                                      // bfloat16 from a float
    uint16_t bits;
    emu_bf16() = default;
    explicit emu_bf16(float f) {
        uint32_t x;
        std::memcpy(&x, &f, 4);
        bits = (x & 0x7fffffffu) > 0x7f800000u ? (uint16_t)((x >> 16) | 0x40u) : (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
    }
};
#define _Float16 emu_half
#define __bf16 emu_bf16

// ---- the state of the running block, and what the entry points report ----
inline std::barrier<>* g_bar;
inline unsigned long long g_slot[1024];                // a collective's operand of every thread of the block
inline std::atomic<int> g_or[2];
inline thread_local int g_phase;
inline unsigned char* g_lds;                           // the launch's dynamic LDS: exactly the bytes it asked for, canaries behind them
inline int g_launches, g_lds_asked, g_lds_overrun;     // launches made | one asked for dynamic LDS | a block wrote past what its launch asked for
#define HIP_DYNAMIC_SHARED(type, var) type* var = reinterpret_cast<type*>(g_lds);
#define KASF_DYNAMIC_LDS(name) float* name = reinterpret_cast<float*>(g_lds)

// ---- barriers and wave collectives (a wave = 64 consecutive threads of a block of up to 1024; each collective costs two barrier phases) ----
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
template <class T> inline T __shfl(T v, int src) {     // from lane src & 63 of the caller's own wave
    static_assert(sizeof(T) <= 8, "");
    unsigned long long raw = 0;
    std::memcpy(&raw, &v, sizeof(T));
    g_slot[threadIdx.x] = raw;
    g_bar->arrive_and_wait();
    const unsigned long long got = g_slot[(threadIdx.x & ~63u) | ((unsigned)src & 63u)];
    g_bar->arrive_and_wait();
    T out;
    std::memcpy(&out, &got, sizeof(T));
    return out;
}
template <class T> inline T __shfl_xor(T v, int off) { return __shfl(v, (int)(threadIdx.x ^ (unsigned)off)); }
inline unsigned long long __ballot(int pred) {         // lanes past the end of the block vote 0
    g_slot[threadIdx.x] = pred != 0;
    g_bar->arrive_and_wait();
    unsigned long long m = 0;
    const unsigned w0 = threadIdx.x & ~63u;
    for (unsigned l = 0; l < 64 && w0 + l < blockDim.x; ++l) m |= (g_slot[w0 + l] & 1ull) << l;
    g_bar->arrive_and_wait();
    return m;
}

// ---- launch: a 2-D grid of 1-D blocks, the shape of every kernel here (a 1-D grid is the y = 1 case) ----
template <class F> void emul_launch(F f, dim3 grid, dim3 block, size_t lds_bytes) {
    ++g_launches;
    g_lds_asked |= lds_bytes != 0;
    std::vector<unsigned char> lds(lds_bytes + 64, 0xA5);
    g_lds = lds.data();
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::barrier<> bar(block.x);
            g_bar = &bar;
            g_or[0].store(0);
            g_or[1].store(0);
            std::vector<std::thread> th;
            for (unsigned l = 0; l < block.x; ++l)
                th.emplace_back([=]() { threadIdx = dim3(l, 0, 0); blockIdx = dim3(bx, by, 0); gridDim = grid; blockDim = block; g_phase = 0; f(); });
            for (auto& t : th) t.join();
            for (size_t i = lds_bytes; i < lds.size(); ++i) g_lds_overrun |= lds[i] != 0xA5;
        }
    g_lds = nullptr;
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) emul_launch([=]() { kern(__VA_ARGS__); }, dim3(grid), dim3(block), (lds))
