// What the C entry points (engine.hip, api_video.hip, api_ops.hip) share: how an entry ends, how a refusal is worded, and the checks that more than one entry makes.
// C++ linkage, inline only: nothing here is exported.  A refuse_* helper returns 0, or sets kasf_last_error() to "who: why" and returns 2; an entry calls them in the
// order of its own checks (tests/test_refusals_cpu.py holds every message, code and the order to tests/golden/refusals.json).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>

#include "kasf.h"
#include "kernels.h"

#define HIPCHK(x)                                                                           \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) return kasf_set_error(1000 + (int)e_, hipGetErrorString(e_)); \
    } while (0)

// the tail of every entry: what the launches left in HIP's error state, else rc
inline int api_done(int rc = 0) {
    HIPCHK(hipGetLastError());
    return rc;
}
// around launchers that report through kasf_set_error: clear before, 3 behind them if one of them spoke
inline void api_clear_error() { kasf_set_error(0, ""); }
inline int api_launchers_spoke() { return kasf_last_error()[0] != '\0' ? 3 : 0; }

inline int refuse(const std::string& who, const std::string& why) { return kasf_set_error(2, (who + ": " + why).c_str()); }
inline int refuse_null() { return kasf_set_error(2, "null pointer argument"); }
inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// name: the parameter as the entry calls it (dtype, out_dtype)
inline int refuse_dtype3(const char* who, const char* name, int32_t dtype) {
    return dtype != KASF_F32 && dtype != KASF_F16 && dtype != KASF_BF16 ? refuse(who, std::string(name) + " must be KASF_DTYPE_F32, _F16 or _BF16") : 0;
}
inline int refuse_frame_size(const char* who, int32_t Hf, int32_t Wf) {
    return Hf < 1 || Hf > 32767 || Wf < 1 || Wf > 32767 ? refuse(who, "Hf and Wf must be in [1, 32767]") : 0;
}
// which: "row" or "output row" of a packed 3-byte-per-pixel frame
inline int refuse_row_stride(const char* who, const char* which, int64_t row_stride, int32_t Wf) {
    return row_stride < (int64_t)3 * Wf ? refuse(who, std::string("the ") + which + " stride must be at least 3 * Wf bytes") : 0;
}
// frame_stride < rows * row_stride, without the product that a huge row stride overflows
inline bool plane_uncovered(int32_t n_frames, int64_t frame_stride, int64_t rows, int64_t row_stride) { return n_frames > 1 && frame_stride / rows < row_stride; }
inline int refuse_plane(const char* who, int32_t n_frames, int64_t frame_stride, int64_t rows, int64_t row_stride) {
    return plane_uncovered(n_frames, frame_stride, rows, row_stride) ? refuse(who, "with more than one frame every frame stride must cover its plane (rows * row stride)") : 0;
}
// the two planes of a 4:2:0 surface; c_min, c_min_text: the least chroma row stride of the entry's layouts, in bytes and in its words
inline int refuse_yuv_rows(const char* who, int64_t y_row_stride, int64_t c_row_stride, int32_t Wf, int64_t c_min, const char* c_min_text) {
    if (y_row_stride < Wf) return refuse(who, "the luma row stride must be at least Wf bytes");
    return c_row_stride < c_min ? refuse(who, std::string("the chroma row stride must be at least ") + c_min_text) : 0;
}
// rows that follow the tracker's output (kasf_stream_track_front, kasf_one_euro_tracked)
inline int refuse_tracked_rows(const char* who, int32_t streams, int32_t track_slots, int32_t rows_mode, int32_t R) {
    if (streams < 1) return refuse(who, "streams must be >= 1");
    if (track_slots < 1 || track_slots > KASF_SORT_MAX) return refuse(who, "track_slots must be in [1, 64]");
    if (R < 1) return refuse(who, "R must be >= 1");
    if (rows_mode != KASF_ROWS_PERSONS && rows_mode != KASF_ROWS_TRACKS) return refuse(who, "rows_mode must be KASF_ROWS_PERSONS or KASF_ROWS_TRACKS");
    return (int64_t)streams * R > INT32_MAX || (int64_t)streams * track_slots > INT32_MAX ? refuse(who, "streams * R and streams * track_slots must fit 32 bits") : 0;
}
// the flip test's left <-> right table: the caller's, or COCO's
inline const int32_t* partner_or_coco(const int32_t* partner) {
    static const int32_t coco_pairs[17] = {0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15};
    return partner ? partner : coco_pairs;
}
inline int refuse_partner(const char* who, const int32_t* pt) {
    for (int j = 0; j < 17; ++j)
        if (pt[j] < 0 || pt[j] > 16) return refuse(who, "partner entries must be in [0, 16]");
    for (int j = 0; j < 17; ++j)
        if (pt[pt[j]] != j) return refuse(who, "partner must be an involution (partner[partner[j]] == j)");
    return 0;
}

// ---- the attention kernels on their own (kasf.h, kasf_op_attention_fwd ... kasf_op_attn_block_fwd) ----
inline int refuse_attn_mode(const char* who, int32_t mode) { return mode != 0 && mode != 1 ? refuse(who, "mode must be 0 (spatial) or 1 (temporal)") : 0; }
// the kernels index tokens x leading dimension in 32 bits: one bound for all of them, at the widest row any of them addresses (384, or a padded leading dimension)
inline bool attn_index_overflows(int32_t batch, int32_t n_frames, int64_t ld = 384) {
    const int64_t frames = (int64_t)batch * n_frames, row = 17 * (ld < 384 ? 384 : ld > ((int64_t)1 << 31) ? (int64_t)1 << 31 : ld);
    return frames > (((int64_t)1 << 31) - 1) / row;          // frames * row >= 2^31, without the product
}
inline int refuse_attn_shape(const char* who, int32_t mode, int32_t batch, int32_t n_frames, int64_t ld = 384) {
    if (int rc = refuse_attn_mode(who, mode)) return rc;
    if (batch < 0) return refuse(who, "batch must be >= 0");
    if (n_frames < 1) return refuse(who, "n_frames must be >= 1");
    return attn_index_overflows(batch, n_frames, ld) ? refuse(who, "batch * n_frames * 17 * max(384, leading dimension) must stay below 2^31") : 0;
}
// name: "ldq", "ldkv", ...; every row is read and written in 16-byte pieces of 8 (bf16) or 4 (fp32) elements
inline int refuse_attn_ld(const char* who, const char* name, int64_t ld) {
    return ld < 128 || ld % 8 != 0 ? refuse(who, std::string(name) + " must be at least 128 (the columns a pointer addresses) and a multiple of 8 elements") : 0;
}

// ---- the prologue, gate, head and embedding kernels on their own (kasf.h, kasf_op_prologue_fwd ... kasf_op_add) ----
inline int refuse_misc_frames(int64_t f) {
    return f < 1 || f * 17 * 384 >= ((int64_t)1 << 31) ? kasf_set_error(2, "frames: 1 <= frames and frames * 17 * 384 < 2^31") : 0;
}
inline int misc_scratch_check(const float* scratch, int64_t floats) {
    if (scratch != nullptr && floats < 1) return kasf_set_error(2, "scratch_floats must be >= 1 with a scratch pointer");
    if (scratch != nullptr && misaligned16(scratch)) return kasf_set_error(2, "scratch must be 16-byte aligned");
    return 0;
}
// scratch != NULL: a local KasfColSink on it and the fixed-order finish on the same stream, as a backward stage does; NULL: the fp32 atomics
struct MiscSink {
    KasfColSink sink;
    KasfColSink* p;
    MiscSink(float* scratch, int64_t floats) : p(scratch != nullptr ? &sink : nullptr) { sink.scratch = scratch; sink.cap = floats; }
    // the finish; error 6 (set by kasf_col_flush) when a launch found the scratch too small and fell back to atomics
    int finish(hipStream_t s) {
        if (p == nullptr) return 0;
        const bool overflow = sink.overflow;
        kasf_col_flush(s, &p, 1);
        return overflow ? 6 : 0;
    }
};
