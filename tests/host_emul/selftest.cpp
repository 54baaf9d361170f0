// The stand-in hip/hip_runtime.h on its own (tests/test_host_emul_cpu.py): toy kernels with known answers, one per thing the header models.
#include <hip/hip_runtime.h>

__global__ void k_indices(int* rec) {                  // the slot is computed from the indices themselves: a wrong index collides or leaves a slot unwritten
    int* r = rec + 9 * ((blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x);
    r[0] = blockIdx.x, r[1] = blockIdx.y, r[2] = threadIdx.x, r[3] = gridDim.x, r[4] = gridDim.y, r[5] = gridDim.z;
    r[6] = blockDim.x, r[7] = blockDim.y, r[8] = blockDim.z;
}
extern "C" void selftest_indices(int* rec) { hipLaunchKernelGGL(k_indices, dim3(3, 2), dim3(128), 0, nullptr, rec); }

__global__ void k_ballot(unsigned long long* out) {
    const unsigned lane = threadIdx.x & 63;
    out[threadIdx.x] = __ballot(threadIdx.x < 64 ? lane % 3 == 0 : lane % 2);
}
extern "C" void selftest_ballot(int threads, unsigned long long* out) { hipLaunchKernelGGL(k_ballot, dim3(1), dim3(threads), 0, nullptr, out); }

__global__ void k_butterfly(float* out) {
    float v = (float)threadIdx.x;
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    out[threadIdx.x] = v;
}
extern "C" void selftest_butterfly(float* out) { hipLaunchKernelGGL(k_butterfly, dim3(1), dim3(128), 0, nullptr, out); }

__global__ void k_broadcast(double* out) { out[threadIdx.x] = __shfl(1000.0 * (threadIdx.x >> 6) + (threadIdx.x & 63) + 0.5, 5); }
extern "C" void selftest_broadcast(double* out) { hipLaunchKernelGGL(k_broadcast, dim3(1), dim3(128), 0, nullptr, out); }

__global__ void k_or(int* out) {
    out[3 * threadIdx.x] = __syncthreads_or(threadIdx.x == 77);
    out[3 * threadIdx.x + 1] = __syncthreads_or(0);
    out[3 * threadIdx.x + 2] = __syncthreads_or(1);
}
extern "C" void selftest_or(int* out) { hipLaunchKernelGGL(k_or, dim3(1), dim3(128), 0, nullptr, out); }

__global__ void k_lds(int n_write, int* same) {
    HIP_DYNAMIC_SHARED(unsigned char, bytes)
    KASF_DYNAMIC_LDS(words);
    if (threadIdx.x == 0) *same = (void*)bytes == (void*)words;
    for (int i = threadIdx.x; i < n_write; i += blockDim.x) bytes[i] = (unsigned char)i;
}
// a launch that asks for n_ask bytes and writes the first n_write -> out = { launches, LDS asked for, overrun, both macros name one buffer }
extern "C" void selftest_lds(int n_ask, int n_write, int* out) {
    g_launches = g_lds_asked = g_lds_overrun = 0;
    hipLaunchKernelGGL(k_lds, dim3(2), dim3(64), (size_t)n_ask, nullptr, n_write, out + 3);
    out[0] = g_launches, out[1] = g_lds_asked, out[2] = g_lds_overrun;
}

extern "C" void selftest_convert(const float* in, int64_t n, uint16_t* half, uint16_t* bf16) {
    for (int64_t i = 0; i < n; ++i) half[i] = _Float16(in[i]).bits, bf16[i] = __bf16(in[i]).bits;
}
