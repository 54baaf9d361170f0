// The C entry points of the constant-limb-length stage (kasf.h, kasf_bone_*).  Each checks its arguments with api_check.h's helpers and calls the launchers of
// k_bones.hip.  Every refusal returns before any device call (tests/test_bones_refusals_cpu.py holds every message here to a case).
#include "api_check.h"

extern "C" {

static int refuse_bone_sizes(int64_t N, int32_t P) {
    if (N < 0 || P < 0) return refuse("bones", "N and P must be >= 0");
    return N > INT32_MAX ? refuse("bones", "N must be below 2^31") : 0;
}
static int refuse_bone_window(int32_t window) { return window < 1 || window > (1 << 20) ? refuse("bones", "window must be in [1, 2^20]") : 0; }

int kasf_bone_median(const float* poses, const int64_t* offsets, int64_t N, int32_t P, float* scratch, float* lengths, int32_t* counts, void* stream) {
    if (refuse_bone_sizes(N, P)) return 2;
    if (P == 0) return 0;
    if (!offsets || !lengths || (N > 0 && (!poses || !scratch))) return refuse_null();
    kasf_launch_bone_lengths((hipStream_t)stream, poses, N, scratch);
    kasf_launch_bone_select((hipStream_t)stream, scratch, offsets, N, P, lengths, counts);
    return api_done();
}
int kasf_bone_apply(const float* poses, const int64_t* offsets, int64_t N, int32_t P, const float* lengths, int32_t per_track, int32_t symmetric, float* out,
                    void* stream) {
    if (refuse_bone_sizes(N, P)) return 2;
    if (N == 0) return 0;
    if (!poses || !lengths || !out || (per_track && !offsets)) return refuse_null();
    if (poses == out) return refuse("bones", "out and poses must be distinct arrays");
    kasf_launch_bone_apply((hipStream_t)stream, poses, offsets, N, P, lengths, per_track ? 1 : 0, symmetric ? 1 : 0, out);
    return api_done();
}
int kasf_bone_push(const float* poses, const int32_t* slots, int32_t K, int32_t S, int32_t window, int32_t symmetric, float* len, int32_t* cnt, float* out,
                   void* stream) {
    if (S < 0 || K < 0 || K > S) return refuse("bones", "need 0 <= K <= S");
    if (slots == nullptr && K != 0 && K != S) return refuse("bones", "without slot ids the call covers every slot (K == S)");
    if (refuse_bone_window(window)) return 2;
    if (K == 0) return 0;
    if (!poses || !len || !cnt || !out) return refuse_null();
    kasf_launch_bone_push((hipStream_t)stream, poses, slots, K, S, window, symmetric ? 1 : 0, len, cnt, out);
    return api_done();
}
int kasf_bone_tracked(const float* poses, const int32_t* ids, const int32_t* slot, const int32_t* born, const int32_t* count_b, int32_t streams,
                      int32_t track_slots, int32_t rows_mode, int32_t R, int32_t window, int32_t symmetric, float* len, int32_t* cnt, int32_t* owner, float* out,
                      int32_t* row_slot, void* stream) {
    if (refuse_tracked_rows("bones", streams, track_slots, rows_mode, R)) return 2;
    if (refuse_bone_window(window)) return 2;
    if (!poses || !ids || !slot || !born || !count_b || !len || !cnt || !owner || !out) return refuse_null();
    kasf_launch_bone_tracked((hipStream_t)stream, poses, ids, slot, born, count_b, streams, track_slots, rows_mode, R, window, symmetric ? 1 : 0, len, cnt, owner,
                             out, row_slot);
    return api_done();
}

}  // extern "C"
