// csrc/k_bones.hip compiled for the host (tests/test_bones_host_cpu.py).  The stand-in has no atomicAdd: the select's integer count on its LDS bins is defined
// here, on the host threads that stand for the lanes.
#include "kernels.h"
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#include "k_bones.hip"
extern "C" void emul_lengths(const float* poses, int64_t N, float* scratch) { kasf_launch_bone_lengths(nullptr, poses, N, scratch); }
extern "C" void emul_select(const float* scratch, const int64_t* offsets, int64_t N, int P, float* lengths, int* counts) {
    kasf_launch_bone_select(nullptr, scratch, offsets, N, P, lengths, counts);
}
extern "C" void emul_apply(const float* poses, const int64_t* offsets, int64_t N, int P, const float* lengths, int per_track, int symmetric, float* out) {
    kasf_launch_bone_apply(nullptr, poses, offsets, N, P, lengths, per_track, symmetric, out);
}
extern "C" void emul_push(const float* x, const int* slots, int K, int S, int window, int symmetric, float* len, int* cnt, float* out) {
    kasf_launch_bone_push(nullptr, x, slots, K, S, window, symmetric, len, cnt, out);
}
extern "C" void emul_tracked(const float* x, const int* ids, const int* slot, const int* born, const int* count_b, int B, int S_t, int rows_mode, int R, int window,
                             int symmetric, float* len, int* cnt, int* owner, float* out, int* row_slot) {
    kasf_launch_bone_tracked(nullptr, x, ids, slot, born, count_b, B, S_t, rows_mode, R, window, symmetric, len, cnt, owner, out, row_slot);
}
