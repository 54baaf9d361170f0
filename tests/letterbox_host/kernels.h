// Host stand-in for csrc/kernels.h, for tests/test_letterbox_host_cpu.py only: just what csrc/k_letterbox.hip needs to compile with g++, and a lockstep
// emulation of its workgroups -- one host thread per GPU thread of a block, the blocks of the two-dimensional grid one after the other, a barrier at every
// __syncthreads, the dynamic LDS a host buffer of exactly the bytes the launch asks for with canaries behind it.  That is a faithful model exactly when every
// barrier sits in block-uniform control flow; a barrier in divergent control flow deadlocks here instead of returning garbage.
// The 16-bit output types are two small classes that round a float to nearest even in software (this g++ may have neither _Float16 nor __bf16); every
// standard header is included BEFORE their names are defined as macros.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include <barrier>
#define KASF_F32 0
#define KASF_BF16 1
#define KASF_F16 2
#define __global__
#define __device__
#define __launch_bounds__(x)
typedef void* hipStream_t;
struct dim3 { unsigned x, y; dim3(unsigned a, unsigned b = 1) : x(a), y(b) {} };
struct Idx { unsigned x, y; };
extern thread_local Idx threadIdx, blockIdx, gridDim;
extern std::barrier<>* g_bar;
extern unsigned char* g_lds;
extern int g_lds_overrun;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline int __mul24(int a, int b) { return (int)((unsigned)a << 8) / 256 * ((int)((unsigned)b << 8) / 256); }      // the low 24 bits of each operand, sign-extended
#define HIP_DYNAMIC_SHARED(type, var) type* var = reinterpret_cast<type*>(g_lds);

struct emu_half {                                      // IEEE binary16 from a float, round to nearest even
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
struct emu_bf16 {                                      // bfloat16 from a float, round to nearest even
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

template <class F> void emul_launch(F f, dim3 grid, unsigned nthreads, size_t lds_bytes) {
    std::vector<unsigned char> lds(lds_bytes + 64, 0xA5);
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            std::barrier<> bar(nthreads);
            g_bar = &bar;
            g_lds = lds.data();
            std::vector<std::thread> th;
            for (unsigned l = 0; l < nthreads; ++l)
                th.emplace_back([=]() { threadIdx = Idx{l, 0}; blockIdx = Idx{bx, by}; gridDim = Idx{grid.x, grid.y}; f(); });
            for (auto& t : th) t.join();
            for (size_t i = lds_bytes; i < lds.size(); ++i) g_lds_overrun |= lds[i] != 0xA5;
        }
}
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) emul_launch([=]() { kern(__VA_ARGS__); }, (grid), (block).x, (lds))
