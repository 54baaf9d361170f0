// Which row of a TrackResult continues whose history (kasf.h, kasf_stream_track_front): the one statement of the rule that k_stream_track_front,
// k_one_euro_tracked and k_bone_tracked apply, so that a lifter and a filter given the same result agree on every row by construction.
// Plain C++: HIP device code in the library, g++ behind the stand-in hip/hip_runtime.h of tests/host_emul/ in the CPU tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lift_math.h"   // lift_clamp

// rows_mode of the tracker-driven entries; kasf.h gives the callers the same two numbers
#ifndef KASF_ROWS_PERSONS
#define KASF_ROWS_PERSONS 0
#define KASF_ROWS_TRACKS 1
#endif

struct TrackedRow {
    bool valid;      // the row has a history: every test below passed
    int64_t g;       // its state entry b * S_t + slot; b * S_t for an invalid row, so always an index into the [B * S_t] state arrays
    int r;           // its track row, clamped into [0, S_t)
    int id;          // ids[b][r]
    bool restart;    // valid, and the entry starts a new history: its owner is another id, or the track was born this tick
};

// Row k (< R) of stream b.  count_b[b] is clamped to [0, S_t]; the track row is count_b - 1 - k (KASF_ROWS_PERSONS) or k (KASF_ROWS_TRACKS), clamped into
// [0, S_t); the row is valid iff k < count_b, id = ids[b][r] >= 1, s = slot[b][r] in [0, S_t) and no lower row of the stream with an id >= 1 names the same s
// (the lowest row of a slot wins).  Every index formed from a device value is clamped into the arrays the host sized: ids / slot / born [B][S_t], owner [B * S_t].
//
// EVERY thread of the workgroup must call this with the same b and k: the lower rows are looked at one per thread and the verdict is a workgroup-wide vote
// (__syncthreads_or), so the result is uniform.  One lower row per thread needs blockDim.x >= S_t: the entry points keep S_t <= 64, the filters launch 64
// threads and the lifter 256.  Valid rows of a launch have distinct g, so the calling workgroup alone reads and writes entry g.  owner[g] is only read here:
// the caller stores the new owner (and whatever else it keeps per entry) behind a __syncthreads() of its own, after every thread has returned from here.
__device__ inline TrackedRow tracked_row(const int* __restrict__ ids, const int* __restrict__ slot, const int* __restrict__ born, const int* __restrict__ count_b,
                                         int b, int k, int S_t, int rows_mode, const int* owner) {
    const int cb = (int)lift_clamp(count_b[b], 0, S_t);
    const int* ids_b = ids + (int64_t)b * S_t;
    const int* slot_b = slot + (int64_t)b * S_t;
    const auto track_row = [&](int row) { return (int)lift_clamp(rows_mode == KASF_ROWS_PERSONS ? cb - 1 - row : row, 0, S_t - 1); };
    TrackedRow t;
    t.r = track_row(k);
    t.id = ids_b[t.r];
    const int s = slot_b[t.r];
    t.valid = k < cb && t.id >= 1 && s >= 0 && s < S_t;
    bool hit = false;
    if (t.valid && (int)threadIdx.x < k) {
        const int r2 = track_row((int)threadIdx.x);
        hit = ids_b[r2] >= 1 && slot_b[r2] == s;
    }
    if (__syncthreads_or(hit ? 1 : 0)) t.valid = false;
    t.g = (int64_t)b * S_t + (t.valid ? s : 0);
    t.restart = t.valid && (owner[t.g] != t.id || born[(int64_t)b * S_t + t.r] != 0);
    return t;
}
