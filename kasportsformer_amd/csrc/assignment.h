// The optimal assignment of one wavefront (kasf.h, kasf_match_groups): the method csrc/k_track.hip describes, restated as a routine over a cost matrix in LDS so
// that the matcher -- and later the tracker -- can call it.  Shortest augmenting paths with dual variables (the method scipy's linear_sum_assignment uses),
// rows = the smaller side, lane = column.  Row quantities (u, col4row, "in the tree") live in the lane of the row, column quantities (v, shortest path cost,
// predecessor, row4col, "scanned") in the lane of the column; a wave-uniform row or column is read with __shfl.  The per-step minimum over unscanned columns is
// a six-step __shfl_xor butterfly over the totally ordered key (cost, column already assigned, lane), so every lane ends with the same winner and exact ties
// resolve the same way on every run.  Every entry of the matrix must be finite.  Every branch around a collective is wave-uniform.
// Plain C++: HIP device code in the library, g++ behind the stand-in hip/hip_runtime.h of tests/host_emul/ in the CPU tests.
#pragma once
#include <hip/hip_runtime.h>

constexpr int ASSIGN_LD = 65;                                  // the row pitch in doubles: odd, so that the transposed walk is conflict-free too

// M[a * ASSIGN_LD + b] = the cost of pairing a with b, a < na <= 64, b < nb <= 64, na, nb >= 1.  Called by all 64 lanes of a one-wavefront workgroup.
// Lane a < na gets b_of_a, lane b < nb gets a_of_b (-1: not assigned; min(na, nb) pairs are made, with the least total cost); the other lanes get -1.
__device__ inline void assign_wave64(const double* M, int na, int nb, int& b_of_a, int& a_of_b) {
    const double inf = __builtin_huge_val();
    const int lane = threadIdx.x;
    const bool tr = na > nb;                                   // rows = the smaller side
    const int nr = tr ? nb : na, nc = tr ? na : nb;
    double u = 0.0, v = 0.0;
    int col4row = -1, row4col = -1;
    for (int cur = 0; cur < nr; ++cur) {
        double spc = inf, minval = 0.0;
        int path = -1, i = cur, sink = -1;
        bool sc = false, sr = false;
        for (int it = 0; it < 65 && sink < 0; ++it) {
            if (lane == i) sr = true;
            const double ui = __shfl(u, i);
            double bv = inf;
            if (lane < nc && !sc) {
                const double c = tr ? M[lane * ASSIGN_LD + i] : M[i * ASSIGN_LD + lane];
                const double r = minval + c - ui - v;
                if (r < spc) { spc = r; path = i; }
                bv = spc;
            }
            int bk = (lane < nc && !sc ? (row4col >= 0 ? 64 : 0) : 128) + lane;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(bv, off);
                const int ok = __shfl_xor(bk, off);
                if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
            }
            if (bk >= 128) break;                              // no column left: cannot happen with nr <= nc and finite costs
            const int j = bk & 63;
            minval = bv;
            const int r4c = __shfl(row4col, j);
            if (r4c < 0) sink = j; else i = r4c;
            if (lane == j) sc = true;
        }
        if (sink < 0) break;
        const double sp = __shfl(spc, col4row < 0 ? 0 : col4row);
        if (lane == cur) u += minval;
        else if (sr) u += minval - sp;
        if (sc) v -= minval - spc;
        for (int j = sink, it = 0; it < 65; ++it) {
            const int ii = __shfl(path, j);
            if (lane == j) row4col = ii;
            const int old = __shfl(col4row, ii);
            if (lane == ii) col4row = j;
            j = old;
            if (ii == cur) break;
        }
    }
    a_of_b = tr ? col4row : row4col;
    b_of_a = tr ? row4col : col4row;
    if (lane >= nb) a_of_b = -1;
    if (lane >= na) b_of_a = -1;
}
