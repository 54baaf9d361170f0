// Lifting a 2-D keypoint track to 3-D (demo/demo.py:194-254, lift_3d_pose): cut the track into T-frame windows, normalise and mirror them
// (demo/lib/utils.py:5-20), and, after the model's forward, merge the flip-TTA pair and put every window's frames back on the track.
// Every kernel here moves 51 floats per frame: HBM-bound, one fp32 element per thread, consecutive threads on consecutive output floats.
// Three forms: one track layout for all persons, many tracks of different lengths packed back to back, and one new frame per tick (k_stream_*).
// The tracks are in the H36M-17 joint layout; COCO-17 detector keypoints are converted in front of these kernels, and the poses they give are taken to
// world space behind them, by k_pose.hip (kasf_coco_h36m / kasf_pose_world).
//
// Window plan (kasportsformer_amd/lift.py window_plan, kasf.h): W windows of T frames over an n-frame track.
//   stride == T (the demo's turn_into_clips, demo.py:138-156): windows start at 0, T, 2T, ...; a last window of L < T frames is resampled to
//     T frames through the host's table resample[T] (demo.py:132-136), and on the way back frame j of it reads position first_pos[j].
//   stride < T, n > T: windows start at 0, s, 2s, ... while start + T < n, plus one at n - T; all full; a frame's output is the mean over the
//     windows that cover it, summed in ascending window order.
//   n <= T (either mode): one window of L = n frames, resampled when n < T.
#include "kernels.h"

namespace {

// utils/utilities.py:128-135 / demo/lib/utils.py:5-13: destination joint j takes source joint c_lift_flip_src[j]; left [1,2,3,14,15,16] <-> right [4,5,6,11,12,13]
__constant__ int c_lift_flip_src[17] = {0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13};

// First frame of window w (of W) on the track.
__device__ inline int64_t lift_start(int64_t w, int64_t W, int64_t n, int T, int stride) {
    return (stride < T && n > T && w == W - 1) ? n - T : w * stride;
}

// x [(1+flip) * P * W, T, 17, 3]: clip (h * P + p) * W + w is window w of person p, mirrored when h == 1.
// x / w * 2 in fp32, then the fp64 subtraction of [1, h / w], stored as fp32 (normalize_screen_coordinates, demo/lib/utils.py:16-20); confidence unchanged.
__global__ __launch_bounds__(256) void k_lift_windows(const float* __restrict__ track, int64_t n, int64_t W, int T, int stride, const int* __restrict__ resample,
                                                      float width, double shift_y, int64_t clips_per_half, int64_t total, float* __restrict__ x) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t clip = i / clip_floats, r = i - clip * clip_floats;
        const int t = (int)(r / 51), q = (int)(r - (int64_t)t * 51), j = q / 3, c = q - 3 * j;
        const bool mirrored = clip >= clips_per_half;
        const int64_t pw = mirrored ? clip - clips_per_half : clip;
        const int64_t p = pw / W, w = pw - p * W;
        const int64_t start = lift_start(w, W, n, T, stride);
        const int64_t L = n - start < T ? n - start : T;
        int64_t f = t;
        if (L < T) {                                   // the resampled window: table entries are clamped into it, a bad table never reads outside the track
            const int64_t rt = resample[t];
            f = rt < 0 ? 0 : (rt >= L ? L - 1 : rt);
        }
        const int js = mirrored ? c_lift_flip_src[j] : j;
        float v = track[(p * n + start + f) * 51 + 3 * js + c];
        if (c < 2) {
            const float scaled = v / width * 2.0f;
            v = (float)((double)scaled - (c == 0 ? 1.0 : shift_y));
            if (mirrored && c == 0) v = -v;
        }
        x[i] = v;
    }
}

// out [P, n, 17, 3] from pred [(1+flip) * P * W, T, 17, 3]: per covering window (p + joint_flip(p_f)) / 2 with the root zeroed (kasf_tta_merge,
// train_and_evaluate_sp.py:46-55 / demo.py:229-235), summed over the covering windows in ascending order and divided by their number.
__global__ __launch_bounds__(256) void k_lift_stitch(const float* __restrict__ pred, int flip, int64_t n, int64_t W, int T, int stride,
                                                     const int* __restrict__ first_pos, int64_t clips_per_half, int64_t total, float* __restrict__ out) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / 51;
        const int q = (int)(i - row * 51), j = q / 3, c = q - 3 * j;
        const int64_t p = row / n, f = row - p * n;
        if (j == 0) {
            out[i] = 0.0f;
            continue;
        }
        // windows covering frame f: the regular ones (start w * stride) in [w_lo, w_hi], then, in overlap mode, the last one (start n - T) when it reaches f
        const bool tail = stride < T && n > T;
        const int64_t w_lo = f < T ? 0 : (f - T) / stride + 1, last_regular = tail ? W - 2 : W - 1;
        const int64_t w_hi = f / stride < last_regular ? f / stride : last_regular;
        float acc = 0.0f;
        int cnt = 0;
        for (int64_t w = w_lo; w <= w_hi + (tail && f >= n - T ? 1 : 0); ++w) {
            const int64_t start = w > w_hi ? n - T : w * stride;
            const int64_t L = n - start < T ? n - start : T;
            int64_t t = f - start;
            if (L < T) {
                const int64_t ft = first_pos[t];
                t = ft < 0 ? 0 : (ft >= T ? T - 1 : ft);
            }
            const int64_t o = (p * W + (w > w_hi ? W - 1 : w)) * clip_floats + t * 51;
            float v = pred[o + q];
            if (flip) {
                const float fv = pred[clips_per_half * clip_floats + o + 3 * c_lift_flip_src[j] + c];
                v = (v + (c == 0 ? -fv : fv)) / 2;
            }
            acc += v;
            ++cnt;
        }
        out[i] = acc / (float)cnt;
    }
}

// ---- many tracks of different lengths in one launch (kasf.h, kasf_lift_*_ragged) ----
// Tracks packed back to back: track p is rows [offsets[p], offsets[p + 1]) of [frames, 17, 3] and owns windows [win_first[p], win_first[p + 1]) of the
// call, cut by its own plan (n = its length, W = its window count).  The two kernels are k_lift_windows / k_lift_stitch with (n, W) taken per track.
// Every index formed from a device table is clamped into the arrays the host sized (frames, windows, tracks): an inconsistent table gives wrong values,
// never an access outside track, pred or the tables.

// The p in [0, P) with sorted[p] <= key < sorted[p + 1] (sorted: P + 1 non-decreasing entries); any table content gives some p in [0, P).
__device__ inline int lift_track_of(const int64_t* __restrict__ sorted, int P, int64_t key) {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sorted[mid] <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline int64_t lift_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// x [(1+flip) * windows, T, 17, 3]: clip h * windows + win_first[p] + w is window w of track p, mirrored when h == 1; track p normalised with width[p], height[p].
__global__ __launch_bounds__(256) void k_lift_windows_ragged(const float* __restrict__ track, int64_t frames, const int64_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ win_first, int P, int64_t windows, const float* __restrict__ width,
                                                             const float* __restrict__ height, int T, int stride, const int* __restrict__ resample,
                                                             int64_t total, float* __restrict__ x) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t clip = i / clip_floats, r = i - clip * clip_floats;
        const int t = (int)(r / 51), q = (int)(r - (int64_t)t * 51), j = q / 3, c = q - 3 * j;
        const bool mirrored = clip >= windows;
        const int64_t g = mirrored ? clip - windows : clip;
        const int p = lift_track_of(win_first, P, g);
        const int64_t base = offsets[p], n = offsets[p + 1] - base, W = win_first[p + 1] - win_first[p], w = g - win_first[p];
        const int64_t start = lift_start(w, W, n, T, stride);
        const int64_t L = n - start < T ? n - start : T;
        int64_t f = t;
        if (L < T) {
            const int64_t rt = resample[(int64_t)p * T + t];
            f = rt < 0 ? 0 : (rt >= L ? L - 1 : rt);
        }
        const int js = mirrored ? c_lift_flip_src[j] : j;
        float v = track[lift_clamp(base + start + f, 0, frames - 1) * 51 + 3 * js + c];
        if (c < 2) {
            const float wp = width[p];
            const float scaled = v / wp * 2.0f;
            v = (float)((double)scaled - (c == 0 ? 1.0 : (double)height[p] / (double)wp));
            if (mirrored && c == 0) v = -v;
        }
        x[i] = v;
    }
}

// out [frames, 17, 3] from pred [(1+flip) * windows, T, 17, 3] in the clip order above: k_lift_stitch's loop over the windows of the frame's track.
__global__ __launch_bounds__(256) void k_lift_stitch_ragged(const float* __restrict__ pred, int flip, int64_t windows, const int64_t* __restrict__ offsets,
                                                            const int64_t* __restrict__ win_first, int P, int T, int stride, const int* __restrict__ first_pos,
                                                            int64_t total, float* __restrict__ out) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / 51;
        const int q = (int)(i - row * 51), j = q / 3, c = q - 3 * j;
        if (j == 0) {
            out[i] = 0.0f;
            continue;
        }
        const int p = lift_track_of(offsets, P, row);
        const int64_t n = offsets[p + 1] - offsets[p], f = row - offsets[p], wb = win_first[p], W = win_first[p + 1] - wb;
        const bool tail = stride < T && n > T;
        const int64_t w_lo = f < T ? 0 : (f - T) / stride + 1, last_regular = tail ? W - 2 : W - 1;
        const int64_t w_hi = f / stride < last_regular ? f / stride : last_regular;
        float acc = 0.0f;
        int cnt = 0;
        for (int64_t w = w_lo; w <= w_hi + (tail && f >= n - T ? 1 : 0); ++w) {
            const int64_t start = w > w_hi ? n - T : w * stride;
            const int64_t L = n - start < T ? n - start : T;
            int64_t t = lift_clamp(f - start, 0, T - 1);
            if (L < T) {
                const int64_t ft = first_pos[(int64_t)p * T + t];
                t = ft < 0 ? 0 : (ft >= T ? T - 1 : ft);
            }
            const int64_t o = lift_clamp(wb + (w > w_hi ? W - 1 : w), 0, windows - 1) * clip_floats + t * 51;
            float v = pred[o + q];
            if (flip) {
                const float fv = pred[windows * clip_floats + o + 3 * c_lift_flip_src[j] + c];
                v = (v + (c == 0 ? -fv : fv)) / 2;
            }
            acc += v;
            ++cnt;
        }
        out[i] = acc / (float)cnt;
    }
}

// ---- one new frame per tick (kasf.h, kasf_stream_*): per-slot history that stays on the device ----
// A slot is one tracked player: ring [S, T, 17, 3] holds the raw pixel keypoints of its last T frames (frame number c at position c % T), count [S] the
// frames pushed since its reset.  Its current window is the last L = min(count, T) frames; a window of L < T frames is the demo's one resampled clip of an
// L-frame track.  resample_tab / first_pos_tab [T + 1][T] hold window_plan(L, T)'s tables in row L (row T: the identity), so no plan is made per tick.
// slots [K] names the slots of a call (NULL: slot i for row i).  As above, every index formed from a device array (slot id, count, table entry) is clamped
// into the arrays the host sized; a count below 1 is read as 1 (below 0 as 0 where a frame is stored), so no % T sees a negative number.

__device__ inline int64_t stream_slot(const int* __restrict__ slots, int64_t i, int S) { return slots ? lift_clamp(slots[i], 0, S - 1) : lift_clamp(i, 0, S - 1); }

// One workgroup per pushed slot: row i of frames [K, 17, 3] goes to ring[slot][count[slot] % T], then count[slot] += 1.  Every thread reads the count before
// the barrier, one thread stores the new one after it.  The slots of a call are distinct (the host checks), so no other workgroup touches this slot.
__global__ __launch_bounds__(256) void k_stream_push(const float* __restrict__ frames, const int* __restrict__ slots, int K, int S, int T,
                                                     float* __restrict__ ring, int64_t* __restrict__ count) {
    for (int64_t i = blockIdx.x; i < K; i += gridDim.x) {
        const int64_t slot = stream_slot(slots, i, S);
        int64_t k = count[slot];
        __syncthreads();
        if (k < 0) k = 0;
        if (threadIdx.x < 51) ring[(slot * T + k % T) * 51 + threadIdx.x] = frames[i * 51 + threadIdx.x];
        if (threadIdx.x == 0) count[slot] = k + 1;
    }
}

// x [(1+flip) * K, T, 17, 3]: clip h * K + i is the current window of slot i of the call, mirrored when h == 1; k_lift_windows_ragged's arithmetic with the
// slot's width and height.  Clip frame t is window frame resample_tab[L][t], i.e. ring position (k - L + that) % T.
__global__ __launch_bounds__(256) void k_stream_windows(const float* __restrict__ ring, const int64_t* __restrict__ count, const int* __restrict__ slots,
                                                        int64_t K, int S, int T, const float* __restrict__ width, const float* __restrict__ height,
                                                        const int* __restrict__ resample_tab, int64_t total, float* __restrict__ x) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t clip = i / clip_floats, r = i - clip * clip_floats;
        const int t = (int)(r / 51), q = (int)(r - (int64_t)t * 51), j = q / 3, c = q - 3 * j;
        const bool mirrored = clip >= K;
        const int64_t slot = stream_slot(slots, mirrored ? clip - K : clip, S);
        const int64_t kc = count[slot], k = kc < 1 ? 1 : kc, L = k < T ? k : T;
        const int64_t f = lift_clamp(resample_tab[L * T + t], 0, L - 1);
        const int js = mirrored ? c_lift_flip_src[j] : j;
        float v = ring[(slot * T + (k - L + f) % T) * 51 + 3 * js + c];
        if (c < 2) {
            const float wp = width[slot];
            const float scaled = v / wp * 2.0f;
            v = (float)((double)scaled - (c == 0 ? 1.0 : (double)height[slot] / (double)wp));
            if (mirrored && c == 0) v = -v;
        }
        x[i] = v;
    }
}

// out [K, n_out, 17, 3] from pred [(1+flip) * K, T, 17, 3] in the clip order above: row r of slot i is window frame clamp(L - 1 - back + r, 0, L - 1), read at
// clip position first_pos_tab[L][that] and merged as k_lift_stitch merges a frame that one window covers.
__global__ __launch_bounds__(256) void k_stream_emit(const float* __restrict__ pred, int flip, const int64_t* __restrict__ count, const int* __restrict__ slots,
                                                     int64_t K, int S, int T, const int* __restrict__ first_pos_tab, int back, int n_out, int64_t total,
                                                     float* __restrict__ out) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / 51;
        const int q = (int)(i - row * 51), j = q / 3, c = q - 3 * j;
        if (j == 0) {
            out[i] = 0.0f;
            continue;
        }
        const int64_t g = row / n_out, r = row - g * n_out;
        const int64_t kc = count[stream_slot(slots, g, S)], k = kc < 1 ? 1 : kc, L = k < T ? k : T;
        const int64_t jw = lift_clamp(L - 1 - back + r, 0, L - 1);
        const int64_t t = lift_clamp(first_pos_tab[L * T + jw], 0, T - 1);
        const int64_t o = g * clip_floats + t * 51;
        float v = pred[o + q];
        if (flip) {
            const float fv = pred[K * clip_floats + o + 3 * c_lift_flip_src[j] + c];
            v = (v + (c == 0 ? -fv : fv)) / 2;
        }
        out[i] = 0.0f + v;                             // k_lift_stitch's sum over the one covering window, divided by 1
    }
}

inline unsigned grid_for(int64_t n) {
    int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace

void kasf_launch_lift_windows(hipStream_t s, const float* track, int P, int64_t n, float width, float height, int T, int stride, const int* resample, int flip,
                              float* x) {
    const int64_t W = kasf_lift_window_count_of(n, T, stride);
    const int64_t per_half = (int64_t)P * W, total = (flip ? 2 : 1) * per_half * T * 51;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_lift_windows, dim3(grid_for(total)), dim3(256), 0, s, track, n, W, T, stride, resample, width, (double)height / (double)width,
                       per_half, total, x);
}

void kasf_launch_lift_stitch(hipStream_t s, const float* pred, int flip, int P, int64_t n, int T, int stride, const int* first_pos, float* out) {
    const int64_t W = kasf_lift_window_count_of(n, T, stride);
    const int64_t total = (int64_t)P * n * 51;
    if (total <= 0 || W <= 0) return;
    hipLaunchKernelGGL(k_lift_stitch, dim3(grid_for(total)), dim3(256), 0, s, pred, flip, n, W, T, stride, first_pos, (int64_t)P * W, total, out);
}

void kasf_launch_lift_windows_ragged(hipStream_t s, const float* track, int64_t frames, const int64_t* offsets, const int64_t* win_first, int P,
                                     int64_t windows, const float* width, const float* height, int T, int stride, const int* resample, int flip, float* x) {
    const int64_t total = (flip ? 2 : 1) * windows * T * 51;
    if (total <= 0 || P <= 0 || frames <= 0) return;
    hipLaunchKernelGGL(k_lift_windows_ragged, dim3(grid_for(total)), dim3(256), 0, s, track, frames, offsets, win_first, P, windows, width, height, T, stride,
                       resample, total, x);
}

void kasf_launch_lift_stitch_ragged(hipStream_t s, const float* pred, int flip, int64_t windows, const int64_t* offsets, const int64_t* win_first, int P,
                                    int64_t frames, int T, int stride, const int* first_pos, float* out) {
    const int64_t total = frames * 51;
    if (total <= 0 || P <= 0 || windows <= 0) return;
    hipLaunchKernelGGL(k_lift_stitch_ragged, dim3(grid_for(total)), dim3(256), 0, s, pred, flip, windows, offsets, win_first, P, T, stride, first_pos, total, out);
}

void kasf_launch_stream_push(hipStream_t s, const float* frames, const int* slots, int K, int S, int T, float* ring, int64_t* count) {
    if (K <= 0 || S <= 0) return;
    hipLaunchKernelGGL(k_stream_push, dim3(K > 4096 ? 4096 : K), dim3(256), 0, s, frames, slots, K, S, T, ring, count);
}

void kasf_launch_stream_windows(hipStream_t s, const float* ring, const int64_t* count, const int* slots, int K, int S, int T, const float* width,
                                const float* height, const int* resample_tab, int flip, float* x) {
    const int64_t total = (flip ? 2 : 1) * (int64_t)K * T * 51;
    if (total <= 0 || S <= 0) return;
    hipLaunchKernelGGL(k_stream_windows, dim3(grid_for(total)), dim3(256), 0, s, ring, count, slots, (int64_t)K, S, T, width, height, resample_tab, total, x);
}

void kasf_launch_stream_emit(hipStream_t s, const float* pred, int flip, const int64_t* count, const int* slots, int K, int S, int T, const int* first_pos_tab,
                             int back, int n_out, float* out) {
    const int64_t total = (int64_t)K * n_out * 51;
    if (total <= 0 || S <= 0) return;
    hipLaunchKernelGGL(k_stream_emit, dim3(grid_for(total)), dim3(256), 0, s, pred, flip, count, slots, (int64_t)K, S, T, first_pos_tab, back, n_out, total, out);
}
