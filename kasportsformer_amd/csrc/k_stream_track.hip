// The stream lifter's slots driven by the tracker's output, on the device (kasf.h, kasf_stream_track_*): what k_lift.hip's k_stream_push + k_stream_windows do
// for slot ids the host uploaded, here for slots, births and deaths read from the TrackResult of k_track.hip -- one launch per tick in front of the model's
// forward, one behind it, nothing read back.
//
// The row rule below is tracked_rows.h's, the one statement the two filters' tracked kernels apply as well.
//
// State per stream b and tracker slot s, g = b * S_t + s: ring [B * S_t, T, 17, 3] and count [B * S_t] as k_lift.hip keeps them, owner [B * S_t] the track id
// whose history the slot holds.  Row k of stream b takes track row r = count_b - 1 - k (rows_mode 0, the order of TrackResult.persons) or r = k (rows_mode 1,
// the order of TrackResult.boxes), count_b clamped to [0, S_t].  The row is valid iff k < min(count_b, R), id = ids[b][r] >= 1, s = slot[b][r] in [0, S_t) and no
// lower row of the stream that passes those three tests has the same s.  A valid row whose owner[g] != id or whose born[b][r] != 0 starts the slot again
// (count 0, owner id); then the frame goes to ring[g][count % T], count += 1, and the row's clips are the slot's current window exactly as k_stream_windows
// writes them.  An invalid row touches no state and gets clips of zeros.
//
// Valid rows of a launch have distinct g, so every ring / count / owner entry is read and written by one workgroup only: no atomics, no hand-off between
// workgroups, the same bits from run to run.  Every index formed from a device value (count_b, slot, count, table entry) is clamped into the arrays the host sized.
// The clip value and the flip-TTA merge are lift_math.h's, the ones k_lift.hip's kernels compute with.
#include "kernels.h"

namespace {

// Float e of a clip of the slot whose count is k (>= 1, the new frame included) and window length L.  The window's newest frame is read from the caller's
// frame, the older ones from ring positions this launch does not write.
__device__ inline float track_clip_value(const float* ring_slot, const float* __restrict__ frame, const int* __restrict__ resample_row, int64_t k, int64_t L, int T,
                                         float wp, float hp, bool mirrored, int e) {
    const int t = e / 51, q = e - t * 51, j = q / 3, c = q - 3 * j;
    const int64_t f = lift_clamp(resample_row[t], 0, L - 1);
    return lift_clip_value(f == L - 1 ? frame : ring_slot, f == L - 1 ? 0 : ((k - L + f) % T) * 51, j, c, wp, (double)hp / (double)wp, mirrored);
}

// One workgroup per row.  x [(1 + flip) * n_rows, T, 17, 3]: clip h * n_rows + row, h == 1 mirrored.  ring is read and written here, so it carries no __restrict__.
__global__ __launch_bounds__(256) void k_stream_track_front(const float* __restrict__ frames, const int* __restrict__ ids, const int* __restrict__ slot,
                                                            const int* __restrict__ born, const int* __restrict__ count_b, int B, int S_t, int rows_mode, int R,
                                                            int T, float* ring, int64_t* count, int* owner, const float* __restrict__ width,
                                                            const float* __restrict__ height, const int* __restrict__ resample_tab, int flip,
                                                            float* __restrict__ x, int* __restrict__ row_slot) {
    const int64_t n_rows = (int64_t)B * R;
    const int clip_floats = T * 51, halves = flip ? 2 : 1;
    for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const int b = (int)(row / R), k = (int)(row - (int64_t)b * R);
        const TrackedRow tr = tracked_row(ids, slot, born, count_b, b, k, S_t, rows_mode, owner);      // k < R by construction
        const bool valid = tr.valid;
        const int64_t g = tr.g;
        int64_t k0 = 0;
        if (valid && !tr.restart) {                                // this workgroup alone touches entry g in this launch
            k0 = count[g];
            if (k0 < 0) k0 = 0;
        }
        __syncthreads();                                           // every thread has the old count and owner before one thread stores the new ones
        const float* frame = frames + row * 51;
        float* ring_slot = ring + g * T * 51;
        if (valid) {
            if (threadIdx.x < 51) ring_slot[(k0 % T) * 51 + threadIdx.x] = frame[threadIdx.x];
            if (threadIdx.x == 0) {
                count[g] = k0 + 1;
                owner[g] = tr.id;
            }
        }
        if (threadIdx.x == 0) row_slot[row] = valid ? (int)g : -1;
        const int64_t kn = k0 + 1, L = kn < T ? kn : T;
        const int* resample_row = resample_tab + L * T;
        const float wp = width[b], hp = height[b];
        for (int h = 0; h < halves; ++h) {
            float* clip = x + ((int64_t)h * n_rows + row) * clip_floats;
            const bool mirrored = h == 1;
            // clips start at any multiple of 4 bytes: scalars up to the first 16-byte boundary, four floats per store from there, scalars for the rest
            int head = (int)((4 - (((uintptr_t)clip >> 2) & 3)) & 3);
            if (head > clip_floats) head = clip_floats;
            const int n_vec = (clip_floats - head) / 4, tail = head + 4 * n_vec;
            if (valid) {
                for (int e = threadIdx.x; e < head; e += 256) clip[e] = track_clip_value(ring_slot, frame, resample_row, kn, L, T, wp, hp, mirrored, e);
                for (int i = threadIdx.x; i < n_vec; i += 256) {
                    const int e = head + 4 * i;
                    float4 v;
                    v.x = track_clip_value(ring_slot, frame, resample_row, kn, L, T, wp, hp, mirrored, e);
                    v.y = track_clip_value(ring_slot, frame, resample_row, kn, L, T, wp, hp, mirrored, e + 1);
                    v.z = track_clip_value(ring_slot, frame, resample_row, kn, L, T, wp, hp, mirrored, e + 2);
                    v.w = track_clip_value(ring_slot, frame, resample_row, kn, L, T, wp, hp, mirrored, e + 3);
                    *reinterpret_cast<float4*>(clip + e) = v;
                }
                for (int e = tail + threadIdx.x; e < clip_floats; e += 256)
                    clip[e] = track_clip_value(ring_slot, frame, resample_row, kn, L, T, wp, hp, mirrored, e);
            } else {
                for (int e = threadIdx.x; e < head; e += 256) clip[e] = 0.0f;
                for (int i = threadIdx.x; i < n_vec; i += 256) *reinterpret_cast<float4*>(clip + head + 4 * i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                for (int e = tail + threadIdx.x; e < clip_floats; e += 256) clip[e] = 0.0f;
            }
        }
    }
}

// out [n_rows, 17, 3] from pred [(1 + flip) * n_rows, T, 17, 3]: k_stream_emit's merge with n_out = 1 for the rows with row_slot >= 0, zeros for the others;
// valid / ids_out / frames_out [n_rows]: 1, owner[g], count[g], or zeros.
__global__ __launch_bounds__(256) void k_stream_track_emit(const float* __restrict__ pred, int flip, const int64_t* __restrict__ count, const int* __restrict__ owner,
                                                           const int* __restrict__ row_slot, int64_t n_rows, int T, const int* __restrict__ first_pos_tab, int back,
                                                           int64_t total, float* __restrict__ out, unsigned char* __restrict__ valid, int* __restrict__ ids_out,
                                                           int64_t* __restrict__ frames_out) {
    const int64_t clip_floats = (int64_t)T * 51;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / 51;
        const int q = (int)(i - row * 51), j = q / 3, c = q - 3 * j;
        const int g = row_slot[row];
        if (q == 0) {
            valid[row] = g >= 0 ? 1 : 0;
            ids_out[row] = g >= 0 ? owner[g] : 0;
            frames_out[row] = g >= 0 ? count[g] : 0;
        }
        if (j == 0 || g < 0) {
            out[i] = 0.0f;
            continue;
        }
        const int64_t kc = count[g], k = kc < 1 ? 1 : kc, L = k < T ? k : T;
        const int64_t jw = lift_clamp(L - 1 - back, 0, L - 1);
        const int64_t t = lift_clamp(first_pos_tab[L * T + jw], 0, T - 1);
        const int64_t o = row * clip_floats + t * 51;
        out[i] = 0.0f + lift_merge(pred, o, n_rows * clip_floats + o, j, c, flip);    // as k_stream_emit: the sum over the one covering window, divided by 1
    }
}

}  // namespace

void kasf_launch_stream_track_front(hipStream_t s, const float* frames, const int* ids, const int* slot, const int* born, const int* count_b, int B, int S_t,
                                    int rows_mode, int R, int T, float* ring, int64_t* count, int* owner, const float* width, const float* height,
                                    const int* resample_tab, int flip, float* x, int* row_slot) {
    const int64_t n_rows = (int64_t)B * R;
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(k_stream_track_front, dim3((unsigned)(n_rows > 4096 ? 4096 : n_rows)), dim3(256), 0, s, frames, ids, slot, born, count_b, B, S_t, rows_mode,
                       R, T, ring, count, owner, width, height, resample_tab, flip, x, row_slot);
}

void kasf_launch_stream_track_emit(hipStream_t s, const float* pred, int flip, const int64_t* count, const int* owner, const int* row_slot, int64_t n_rows, int T,
                                   const int* first_pos_tab, int back, float* out, unsigned char* valid, int* ids_out, int64_t* frames_out) {
    const int64_t total = n_rows * 51;
    if (total <= 0) return;
    int64_t grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(k_stream_track_emit, dim3((unsigned)grid), dim3(256), 0, s, pred, flip, count, owner, row_slot, n_rows, T, first_pos_tab, back, total, out,
                       valid, ids_out, frames_out);
}
