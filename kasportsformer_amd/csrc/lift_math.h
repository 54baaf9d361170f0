// The window arithmetic every lifting kernel shares (k_lift.hip, k_stream_track.hip; the joint table also k_eval.hip): one definition of the window count, the
// left/right joint table, the clip value, the flip-TTA merge and the mean over the windows that cover a frame.  "Every pose is lift_track of the current
// window" holds bit for bit between the batch, ragged, stream and tracked forms because all of them compute through these functions.
// Plain C++: HIP device code in the library, g++ behind the stand-in hip/hip_runtime.h of tests/host_emul/ (which defines __device__ / __constant__) in the CPU tests.
#pragma once
#include <stdint.h>

// Windows of T frames over an n-frame track: none for n = 0, one for n <= T, else ceil((n - T) / stride) + 1 (stride == T: ceil(n / T)).
inline int64_t kasf_lift_window_count_of(int64_t n, int T, int stride) {
    return n <= 0 ? 0 : (n <= T ? 1 : (n - T + stride - 1) / stride + 1);
}

namespace {
// utils/utilities.py:128-135 / demo/lib/utils.py:5-13: destination joint j takes source joint c_lift_flip_src[j]; left [1,2,3,14,15,16] <-> right [4,5,6,11,12,13].
// A __constant__ array, not a local one: a dynamically indexed local array can go to scratch.
__constant__ int c_lift_flip_src[17] = {0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13};
}  // namespace

__device__ inline int64_t lift_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Component c of joint j of a clip frame cut from the source frame [17,3] at src[o ...] (pixel x, y, confidence): x / w * 2 in fp32, then the fp64 subtraction of
// [1, h / w] (shift_y = (double)h / (double)w), stored as fp32 (normalize_screen_coordinates, demo/lib/utils.py:16-20); a mirrored clip takes the joint's
// left/right partner and negates x (flip_data, demo/lib/utils.py:5-13); confidence unchanged.
__device__ inline float lift_clip_value(const float* src, int64_t o, int j, int c, float width, double shift_y, bool mirrored) {
    float v = src[o + 3 * (mirrored ? c_lift_flip_src[j] : j) + c];
    if (c < 2) {
        const float scaled = v / width * 2.0f;
        v = (float)((double)scaled - (c == 0 ? 1.0 : shift_y));
        if (mirrored && c == 0) v = -v;
    }
    return v;
}

// Component c of joint j of the merged prediction of one clip frame: pred[o ...] is the frame in the plain clip, pred[o_flip ...] the same frame in the
// mirrored clip; (p + joint_flip(p_f)) / 2 (kasf_tta_merge, train_and_evaluate_sp.py:46-55 / demo.py:229-235), or p alone without flip.  The caller zeroes the root.
__device__ inline float lift_merge(const float* __restrict__ pred, int64_t o, int64_t o_flip, int j, int c, int flip) {
    float v = pred[o + 3 * j + c];
    if (flip) {
        const float fv = pred[o_flip + 3 * c_lift_flip_src[j] + c];
        v = (v + (c == 0 ? -fv : fv)) / 2;
    }
    return v;
}

// Component c of joint j of frame f of an n-frame track whose W windows are clips [wb, wb + W) of pred [(1+flip) * windows, T, 17, 3]: the merged values of the
// windows that cover f, summed in ascending window order and divided by their number.  The covering windows are the regular ones (start w * stride) in
// [w_lo, w_hi], then, in overlap mode, the last one (start n - T) when it reaches f; a frame of a resampled window (L < T) is read at clip position
// first_pos[f - start]; the table entry is clamped into [0, T).  kTables: n, W and wb were read from device tables (the ragged form), so the frame position and
// the clip index are clamped into [0, T) and [0, windows) as well -- an inconsistent table gives wrong values, never an access outside pred or first_pos.  With
// host arguments the entry point has checked them, and the two clamps per window cost the uniform stitch kernel 9-13 % on an MI355X.
template <bool kTables>
__device__ inline float lift_cover_mean(const float* __restrict__ pred, int flip, int64_t windows, int64_t f, int64_t n, int64_t W, int64_t wb, int T, int stride,
                                        const int* __restrict__ first_pos, int j, int c) {
    const int64_t clip_floats = (int64_t)T * 51;
    const bool tail = stride < T && n > T;
    const int64_t w_lo = f < T ? 0 : (f - T) / stride + 1, last_regular = tail ? W - 2 : W - 1;
    const int64_t w_hi = f / stride < last_regular ? f / stride : last_regular;
    float acc = 0.0f;
    int cnt = 0;
    for (int64_t w = w_lo; w <= w_hi + (tail && f >= n - T ? 1 : 0); ++w) {
        const int64_t start = w > w_hi ? n - T : w * stride;
        const int64_t L = n - start < T ? n - start : T;
        int64_t t = f - start, clip = wb + (w > w_hi ? W - 1 : w);
        if (kTables) t = lift_clamp(t, 0, T - 1), clip = lift_clamp(clip, 0, windows - 1);
        if (L < T) t = lift_clamp(first_pos[t], 0, T - 1);
        const int64_t o = clip * clip_floats + t * 51;
        acc += lift_merge(pred, o, windows * clip_floats + o, j, c, flip);
        ++cnt;
    }
    return acc / (float)cnt;
}
