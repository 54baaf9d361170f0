// Lifting a 2-D keypoint track to 3-D (demo/demo.py:194-254, lift_3d_pose): cut the track into T-frame windows, normalise and mirror them
// (demo/lib/utils.py:5-20), and, after the model's forward, merge the flip-TTA pair and put every window's frames back on the track.
// Every kernel here moves 51 floats per frame: HBM-bound, one fp32 element per thread, consecutive threads on consecutive output floats.
// Three forms: one track layout for all persons, many tracks of different lengths packed back to back, and one new frame per tick (k_stream_*).
// The tracks are in the H36M-17 joint layout; COCO-17 detector keypoints are converted in front of these kernels, and the poses they give are taken to
// world space behind them, by k_pose.hip (kasf_coco_h36m / kasf_pose_world).
// The arithmetic of all three forms -- clip value, flip-TTA merge, mean over the covering windows -- is written once, in lift_math.h.
//
// Window plan (kasportsformer_amd/lift.py window_plan, kasf.h): W windows of T frames over an n-frame track.
//   stride == T (the demo's turn_into_clips, demo.py:138-156): windows start at 0, T, 2T, ...; a last window of L < T frames is resampled to
//     T frames through the host's table resample[T] (demo.py:132-136), and on the way back frame j of it reads position first_pos[j].
//   stride < T, n > T: windows start at 0, s, 2s, ... while start + T < n, plus one at n - T; all full; a frame's output is the mean over the
//     windows that cover it, summed in ascending window order.
//   n <= T (either mode): one window of L = n frames, resampled when n < T.
#include "kernels.h"

namespace {

// First frame of window w (of W) on the track.
__device__ inline int64_t lift_start(int64_t w, int64_t W, int64_t n, int T, int stride) {
    return (stride < T && n > T && w == W - 1) ? n - T : w * stride;
}

// The p in [0, P) with sorted[p] <= key < sorted[p + 1] (sorted: P + 1 non-decreasing entries); any table content gives some p in [0, P).
__device__ inline int lift_track_of(const int64_t* __restrict__ sorted, int P, int64_t key) {
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sorted[mid] <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// A plan says where the tracks of a call lie: `frames` rows of [17,3] and `windows` clips per half in all; clip g and output row `row` belong to tracks
// clip_track(g) / row_track(row); track p is rows [base, base + n) and clips [wb, wb + W), its resample / first_pos tables start at entry `tab` of the
// call's, and it is normalised with width(p) and shift_y(p) = h / w in fp64.  kTables: the spans are read from device tables, so every index formed from
// them is clamped into the arrays the host sized (frames, windows, tracks) -- an inconsistent table gives wrong values, never an access outside them.
struct LiftSpan { int64_t base, n, wb, W, tab; };

// P persons with one n-frame layout (kasf_lift_windows / _stitch): one table, one resolution, h / w computed by the host.
struct UniformPlan {
    static constexpr bool kTables = false;
    int64_t n, W, frames, windows;
    float w;
    double sy;
    __device__ int64_t clip_track(int64_t g) const { return g / W; }
    __device__ int64_t row_track(int64_t row) const { return row / n; }
    __device__ LiftSpan span(int64_t p) const { return {p * n, n, p * W, W, 0}; }
    __device__ float width(int64_t) const { return w; }
    __device__ double shift_y(int64_t) const { return sy; }
};

// Tracks of different lengths packed back to back (kasf.h, kasf_lift_*_ragged): track p is rows [offsets[p], offsets[p + 1]) and owns windows
// [win_first[p], win_first[p + 1]) of the call, cut by its own plan (n = its length, W = its window count), with row p of the [P, T] tables.
struct RaggedPlan {
    static constexpr bool kTables = true;
    const int64_t* __restrict__ offsets;
    const int64_t* __restrict__ win_first;
    const float* __restrict__ w;
    const float* __restrict__ h;
    int P, T;
    int64_t frames, windows;
    __device__ int64_t clip_track(int64_t g) const { return lift_track_of(win_first, P, g); }
    __device__ int64_t row_track(int64_t row) const { return lift_track_of(offsets, P, row); }
    __device__ LiftSpan span(int64_t p) const { return {offsets[p], offsets[p + 1] - offsets[p], win_first[p], win_first[p + 1] - win_first[p], p * T}; }
    __device__ float width(int64_t p) const { return w[p]; }
    __device__ double shift_y(int64_t p) const { return (double)h[p] / (double)w[p]; }
};

// x [(1+flip) * windows, T, 17, 3]: clip h * windows + wb + w is window w of its track, mirrored when h == 1.
template <class Plan>
__global__ __launch_bounds__(256) void k_lift_windows(const float* __restrict__ track, Plan plan, int T, int stride, const int* __restrict__ resample,
                                                      int64_t total, float* __restrict__ x) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t clip = i / clip_floats, r = i - clip * clip_floats;
        const int t = (int)(r / 51), q = (int)(r - (int64_t)t * 51), j = q / 3, c = q - 3 * j;
        const bool mirrored = clip >= plan.windows;
        const int64_t g = mirrored ? clip - plan.windows : clip, p = plan.clip_track(g);
        const LiftSpan k = plan.span(p);
        const int64_t start = lift_start(g - k.wb, k.W, k.n, T, stride);
        const int64_t L = k.n - start < T ? k.n - start : T;
        int64_t f = t;
        if (L < T) f = lift_clamp(resample[k.tab + t], 0, L - 1);        // the resampled window: a bad table never reads outside it
        const int64_t row = Plan::kTables ? lift_clamp(k.base + start + f, 0, plan.frames - 1) : k.base + start + f;
        x[i] = lift_clip_value(track, row * 51, j, c, plan.width(p), plan.shift_y(p), mirrored);
    }
}

// out [frames, 17, 3] from pred [(1+flip) * windows, T, 17, 3] in the clip order above: the root zeroed, every other float the mean over its covering windows.
template <class Plan>
__global__ __launch_bounds__(256) void k_lift_stitch(const float* __restrict__ pred, int flip, Plan plan, int T, int stride, const int* __restrict__ first_pos,
                                                     int64_t total, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / 51;
        const int q = (int)(i - row * 51), j = q / 3, c = q - 3 * j;
        if (j == 0) {
            out[i] = 0.0f;
            continue;
        }
        const LiftSpan k = plan.span(plan.row_track(row));
        out[i] = lift_cover_mean<Plan::kTables>(pred, flip, plan.windows, row - k.base, k.n, k.W, k.wb, T, stride, first_pos + k.tab, j, c);
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

// x [(1+flip) * K, T, 17, 3]: clip h * K + i is the current window of slot i of the call, mirrored when h == 1, normalised with the slot's width and
// height.  Clip frame t is window frame resample_tab[L][t], i.e. ring position (k - L + that) % T.
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
        const float wp = width[slot];
        x[i] = lift_clip_value(ring, (slot * T + (k - L + f) % T) * 51, j, c, wp, (double)height[slot] / (double)wp, mirrored);
    }
}

// out [K, n_out, 17, 3] from pred [(1+flip) * K, T, 17, 3] in the clip order above: row r of slot i is window frame clamp(L - 1 - back + r, 0, L - 1), read at
// clip position first_pos_tab[L][that] and merged as a frame that one window covers: lift_cover_mean's 0.0f + v, divided by 1.
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
        out[i] = 0.0f + lift_merge(pred, o, K * clip_floats + o, j, c, flip);
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
    const UniformPlan plan{n, W, (int64_t)P * n, per_half, width, (double)height / (double)width};
    hipLaunchKernelGGL(k_lift_windows<UniformPlan>, dim3(grid_for(total)), dim3(256), 0, s, track, plan, T, stride, resample, total, x);
}

void kasf_launch_lift_stitch(hipStream_t s, const float* pred, int flip, int P, int64_t n, int T, int stride, const int* first_pos, float* out) {
    const int64_t W = kasf_lift_window_count_of(n, T, stride);
    const int64_t total = (int64_t)P * n * 51;
    if (total <= 0 || W <= 0) return;
    const UniformPlan plan{n, W, (int64_t)P * n, (int64_t)P * W, 0.0f, 0.0};
    hipLaunchKernelGGL(k_lift_stitch<UniformPlan>, dim3(grid_for(total)), dim3(256), 0, s, pred, flip, plan, T, stride, first_pos, total, out);
}

void kasf_launch_lift_windows_ragged(hipStream_t s, const float* track, int64_t frames, const int64_t* offsets, const int64_t* win_first, int P,
                                     int64_t windows, const float* width, const float* height, int T, int stride, const int* resample, int flip, float* x) {
    const int64_t total = (flip ? 2 : 1) * windows * T * 51;
    if (total <= 0 || P <= 0 || frames <= 0) return;
    const RaggedPlan plan{offsets, win_first, width, height, P, T, frames, windows};
    hipLaunchKernelGGL(k_lift_windows<RaggedPlan>, dim3(grid_for(total)), dim3(256), 0, s, track, plan, T, stride, resample, total, x);
}

void kasf_launch_lift_stitch_ragged(hipStream_t s, const float* pred, int flip, int64_t windows, const int64_t* offsets, const int64_t* win_first, int P,
                                    int64_t frames, int T, int stride, const int* first_pos, float* out) {
    const int64_t total = frames * 51;
    if (total <= 0 || P <= 0 || windows <= 0) return;
    const RaggedPlan plan{offsets, win_first, nullptr, nullptr, P, T, frames, windows};
    hipLaunchKernelGGL(k_lift_stitch<RaggedPlan>, dim3(grid_for(total)), dim3(256), 0, s, pred, flip, plan, T, stride, first_pos, total, out);
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
