// Person boxes -> tracked person boxes (kasf.h, kasf_sort_update): the demo's SORT tracker between the detector and the crop
//   Sort.update, KalmanBoxTracker, associate_detections_to_trackers, iou          demo/lib/sort/sort.py:15-222
//   the empty-frame hold and the num_person oldest tracks of gen_video_kpts         demo/lib/hrnet/gen_kpts.py:125-143
// One launch per tick, one wave64 workgroup per stream, no atomics, no scratch, nothing that depends on the batch: a stream's tick is a function of its
// own state, detections and count alone, and every step is evaluated in one fixed order, so results repeat bit for bit.
// MAPPING.  Lane = position in the track list while tracks are handled (predict, cost column, update, emit, death), lane = detection index while
// detections are handled (validity, births); hence slots <= 64 and max_dets <= 64.  A track lives in registers from the load at the top to the store at the
// bottom: x[7], the 13 numbers of P (with this F, H and a diagonal P0 the covariance keeps the blocks (cx,vx), (cy,vy), (s,vs) and the scalar r; the products
// with the exact zeros and ones of F and H are left out, the remaining operations are the dense form's, in its order) and six counters.  Tracks change
// position only by a ballot prefix: after the predict (a non-finite box leaves) through a register gather, at the end (deaths) through the store address.
// ASSIGNMENT.  Shortest augmenting paths with dual variables (the method scipy's linear_sum_assignment uses), rows = the smaller side, lane = column.  Row
// quantities (u, col4row, "in the tree") live in the lane of the row, column quantities (v, shortest path cost, predecessor, row4col, "scanned") in the lane
// of the column; a wave-uniform row or column is read with __shfl.  The per-step minimum over unscanned columns is a six-step __shfl_xor butterfly over the
// totally ordered key (cost, column already assigned, lane), so every lane ends with the same winner.  The costs -(double)(float)IoU sit in LDS,
// [detection][track] with a row pitch of 65 doubles so that the transposed walk (more detections than tracks) is conflict-free too.
#include "kernels.h"

namespace {

constexpr int TR_LD = 65;
constexpr double TR_INF = __builtin_huge_val();

struct Track {
    double x[7];
    double P[13];          // block k < 3 (cx,vx), (cy,vy), (s,vs): P[4k] = pos-pos, +1 = pos-vel, +2 = vel-pos, +3 = vel-vel; P[12] = r-r
    int id, slot, tsu, hits, streak, age;
};

struct TrackArgs {
    unsigned char* state;
    long long state_stride;
    const float* dets;
    long long det_bstride, det_rstride;
    const int* det_count;
    float* boxes;
    int *ids, *slot, *born, *count, *dropped;
    float* persons;
    int* person_count;
    int S, D, R, max_age, min_hits, num_person, hold_last;
    float thr;
};

__device__ inline bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }       // false for a NaN
__device__ inline bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }
__device__ inline unsigned long long below(int lane) { return (1ull << lane) - 1ull; }
__device__ inline int popc(unsigned long long m) { return __popcll(m); }

__device__ inline void gather(Track& t, int src) {
#pragma unroll
    for (int k = 0; k < 7; ++k) t.x[k] = __shfl(t.x[k], src);
#pragma unroll
    for (int k = 0; k < 13; ++k) t.P[k] = __shfl(t.P[k], src);
    t.id = __shfl(t.id, src); t.slot = __shfl(t.slot, src); t.tsu = __shfl(t.tsu, src);
    t.hits = __shfl(t.hits, src); t.streak = __shfl(t.streak, src); t.age = __shfl(t.age, src);
}

// sort.py:48-58
__device__ inline void state_box(const double* x, double* b) {
    const double w = sqrt(x[2] * x[3]);
    const double h = x[2] / w;
    b[0] = x[0] - w / 2.0; b[1] = x[1] - h / 2.0; b[2] = x[0] + w / 2.0; b[3] = x[1] + h / 2.0;
}

// one (position, velocity) block of P = F P F^T + Q
__device__ inline void predict_block(double* p, double qv) {
    const double a = p[0], b = p[1], c = p[2], d = p[3];
    const double fa = a + c, fb = b + d;                       // row pos of F P; row vel is (c, d)
    p[0] = (fa + fb) + 1.0; p[1] = fb; p[2] = c + d; p[3] = d + qv;
}

// one block of filterpy's update with the measurement on the position: returns through x, v, p
__device__ inline void update_block(double* p, double& xp, double& xv, double z, double r) {
    const double a = p[0], b = p[1], c = p[2], d = p[3];
    const double y = z - xp;
    const double si = 1.0 / (a + r);
    const double kp = a * si, kv = c * si;
    xp = xp + kp * y; xv = xv + kv * y;
    const double m = 1.0 - kp, n = 0.0 - kv;                   // I - K H: (m 0; n 1)
    const double ap0 = m * a, ap1 = m * b, ap2 = n * a + c, ap3 = n * b + d;
    p[0] = ap0 * m + (kp * r) * kp;
    p[1] = (ap0 * n + ap1) + (kp * r) * kv;
    p[2] = ap2 * m + (kv * r) * kp;
    p[3] = (ap2 * n + ap3) + (kv * r) * kv;
}

__global__ __launch_bounds__(64) void k_sort_update(const TrackArgs A) {
    __shared__ double C[64 * TR_LD];
    __shared__ double dbox[64][4];
    __shared__ int perm[64], bsrc[64], freeslot[64];

    const int lane = threadIdx.x, b = blockIdx.x, S = A.S, D = A.D;
    unsigned char* st = A.state + (long long)b * A.state_stride;
    int* hdr = (int*)st;
    double* sx = (double*)(st + KASF_SORT_HEADER_BYTES);
    double* sP = sx + 7 * S;
    int* si = (int*)(sP + 13 * S);
    float* hold = (float*)(si + 6 * S);

    int n = min(max(hdr[0], 0), S);
    int next_id = hdr[1];
    const int frame_count = hdr[2] + 1;
    int hold_n = min(max(hdr[3], 0), D);

    // ---- load and predict (sort.py:104-116) ----
    Track t;
#pragma unroll
    for (int k = 0; k < 7; ++k) t.x[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 13; ++k) t.P[k] = 0.0;
    t.id = t.slot = t.tsu = t.hits = t.streak = t.age = 0;
    double pb[4] = {0.0, 0.0, 0.0, 0.0};
    bool keep = false;
    if (lane < n) {
#pragma unroll
        for (int k = 0; k < 7; ++k) t.x[k] = sx[k * S + lane];
#pragma unroll
        for (int k = 0; k < 13; ++k) t.P[k] = sP[k * S + lane];
        t.id = si[lane]; t.slot = si[S + lane]; t.tsu = si[2 * S + lane]; t.hits = si[3 * S + lane]; t.streak = si[4 * S + lane]; t.age = si[5 * S + lane];
        if ((t.x[6] + t.x[2]) <= 0.0) t.x[6] *= 0.0;
        t.x[0] = t.x[0] + t.x[4]; t.x[1] = t.x[1] + t.x[5]; t.x[2] = t.x[2] + t.x[6];
        predict_block(t.P + 0, 0.01); predict_block(t.P + 4, 0.01); predict_block(t.P + 8, 0.01 * 0.01);
        t.P[12] = t.P[12] + 1.0;
        t.age += 1;
        if (t.tsu > 0) t.streak = 0;
        t.tsu += 1;
        state_box(t.x, pb);
        keep = finite_d(pb[0]) && finite_d(pb[1]) && finite_d(pb[2]) && finite_d(pb[3]) && t.slot >= 0 && t.slot < S;
    }
    {
        const unsigned long long km = __ballot(keep);
        if (popc(km) != n) {                                   // wave-uniform: some track's predicted box is not finite
            if (keep) perm[popc(km & below(lane))] = lane;
            __syncthreads();
            n = popc(km);
            const int src = lane < n ? perm[lane] : lane;
            gather(t, src);
#pragma unroll
            for (int k = 0; k < 4; ++k) pb[k] = __shfl(pb[k], src);
            __syncthreads();
        }
    }

    // ---- detections: the valid ones, in order, as fp64 in LDS; the empty-frame hold ----
    int nd;
    {
        const int raw = A.det_count ? min(max(A.det_count[b], 0), A.R) : A.R;
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        bool ok = false;
        if (lane < raw) {
            const float* row = A.dets + (long long)b * A.det_bstride + (long long)lane * A.det_rstride;
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = row[k];
            ok = finite_f(f[0]) && finite_f(f[1]) && finite_f(f[2]) && finite_f(f[3]) && (double)f[3] - (double)f[1] > 0.0;
        }
        const unsigned long long vm = __ballot(ok);
        nd = popc(vm);
        const int at = popc(vm & below(lane));
        if (ok) {
#pragma unroll
            for (int k = 0; k < 4; ++k) dbox[at][k] = (double)f[k];
        }
        if (A.hold_last) {
            if (nd > 0) {
                if (ok) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) hold[at * 4 + k] = f[k];
                }
                hold_n = nd;
            } else if (hold_n > 0) {
                nd = hold_n;
                if (lane < nd) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) dbox[lane][k] = (double)hold[lane * 4 + k];
                }
            }
        }
        __syncthreads();
    }

    // ---- costs: IoU in fp64, rounded to fp32 (sort.py:16-30,133-137), negated ----
    if (lane < n) {
        const double ta = (pb[2] - pb[0]) * (pb[3] - pb[1]);
        for (int d = 0; d < nd; ++d) {
            const double d0 = dbox[d][0], d1 = dbox[d][1], d2 = dbox[d][2], d3 = dbox[d][3];
            const double w = fmax(0.0, fmin(d2, pb[2]) - fmax(d0, pb[0]));
            const double h = fmax(0.0, fmin(d3, pb[3]) - fmax(d1, pb[1]));
            const double wh = w * h;
            double o = wh / ((d2 - d0) * (d3 - d1) + ta - wh);
            if (!finite_d(o)) o = 0.0;
            C[d * TR_LD + lane] = -(double)(float)o;
        }
    }
    __syncthreads();

    // ---- assignment ----
    int det_of_track = -1, track_of_det = -1;
    if (n > 0 && nd > 0) {
        const bool tr = nd > n;                                // rows = the smaller side
        const int nr = tr ? n : nd, nc = tr ? nd : n;
        double u = 0.0, v = 0.0;
        int col4row = -1, row4col = -1;
        for (int cur = 0; cur < nr; ++cur) {
            double spc = TR_INF, minval = 0.0;
            int path = -1, i = cur, sink = -1;
            bool sc = false, sr = false;
            for (int it = 0; it < 65 && sink < 0; ++it) {
                if (lane == i) sr = true;
                const double ui = __shfl(u, i);
                double bv = TR_INF;
                if (lane < nc && !sc) {
                    const double c = tr ? C[lane * TR_LD + i] : C[i * TR_LD + lane];
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
                if (bk >= 128) break;                          // no column left: cannot happen with nr <= nc and finite costs
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
        det_of_track = tr ? col4row : row4col;
        track_of_det = tr ? row4col : col4row;
        if (lane >= n) det_of_track = -1;
        if (lane >= nd) track_of_det = -1;
    }

    // ---- threshold (sort.py:151-158) and update of the matched tracks ----
    bool low = false;                                          // lane = track: assigned, but below the threshold
    if (det_of_track >= 0) {
        low = (float)(-C[det_of_track * TR_LD + lane]) < A.thr;
        if (!low) {
            const double* z = dbox[det_of_track];
            const double w = z[2] - z[0], h = z[3] - z[1];
            t.tsu = 0; t.hits += 1; t.streak += 1;
            update_block(t.P + 0, t.x[0], t.x[4], z[0] + w / 2.0, 1.0);
            update_block(t.P + 4, t.x[1], t.x[5], z[1] + h / 2.0, 1.0);
            update_block(t.P + 8, t.x[2], t.x[6], w * h, 10.0);
            {
                const double a = t.P[12], y = w / h - t.x[3], sinv = 1.0 / (a + 10.0), k = a * sinv, m = 1.0 - k;
                t.x[3] = t.x[3] + k * y;
                t.P[12] = (m * a) * m + (k * 10.0) * k;
            }
        }
    }
    const bool det_low = __shfl((int)low, track_of_det < 0 ? 0 : track_of_det) != 0 && track_of_det >= 0;      // lane = detection

    // ---- births (sort.py:207-210): the detections outside the assignment first, then the ones unmatched by the threshold ----
    int dropped = 0;
    const int n_before = n;
    {
        unsigned long long used = (lane < n) ? (1ull << t.slot) : 0ull;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) used |= __shfl_xor(used, off);
        const bool is_free = lane < S && !((used >> lane) & 1ull);
        const unsigned long long fm = __ballot(is_free);
        if (is_free) freeslot[popc(fm & below(lane))] = lane;
        const bool g1 = lane < nd && track_of_det < 0, g2 = lane < nd && det_low;
        const unsigned long long m1 = __ballot(g1), m2 = __ballot(g2);
        const int rank = g1 ? popc(m1 & below(lane)) : popc(m1) + popc(m2 & below(lane));
        const int want = popc(m1) + popc(m2), room = S - n;
        const int nb = min(want, room);
        dropped = want - nb;
        if ((g1 || g2) && rank < nb) bsrc[rank] = lane;
        __syncthreads();
        if (lane >= n && lane < n + nb) {
            const int k = lane - n;
            const double* z = dbox[bsrc[k]];
            const double w = z[2] - z[0], h = z[3] - z[1];
            t.x[0] = z[0] + w / 2.0; t.x[1] = z[1] + h / 2.0; t.x[2] = w * h; t.x[3] = w / h; t.x[4] = 0.0; t.x[5] = 0.0; t.x[6] = 0.0;
#pragma unroll
            for (int q = 0; q < 3; ++q) { t.P[4 * q] = 10.0; t.P[4 * q + 1] = 0.0; t.P[4 * q + 2] = 0.0; t.P[4 * q + 3] = 10000.0; }
            t.P[12] = 10.0;
            t.id = next_id + k; t.slot = freeslot[k]; t.tsu = 0; t.hits = 0; t.streak = 0; t.age = 0;
        }
        n += nb;
        next_id += nb;
    }

    // ---- emit, newest first (sort.py:211-216), and the num_person oldest of them (gen_kpts.py:137-141) ----
    {
        const bool emit = lane < n && t.tsu < 1 && (t.streak >= A.min_hits || frame_count <= A.min_hits);
        const unsigned long long em = __ballot(emit);
        const int cnt = popc(em);
        float* ob = A.boxes + (long long)b * S * 4;
        int *oi = A.ids + (long long)b * S, *os = A.slot + (long long)b * S, *on = A.born + (long long)b * S;
        float* op = A.persons + (long long)b * A.num_person * 4;
        const int pc = min(cnt, A.num_person);
        if (emit) {
            double bx[4];
            state_box(t.x, bx);
            const int older = popc(em & below(lane));
            const int row = cnt - 1 - older;
#pragma unroll
            for (int k = 0; k < 4; ++k) ob[row * 4 + k] = (float)bx[k];
            oi[row] = t.id + 1; os[row] = t.slot; on[row] = lane >= n_before ? 1 : 0;
            if (older < A.num_person) {
#pragma unroll
                for (int k = 0; k < 4; ++k) op[older * 4 + k] = (float)bx[k];
            }
        }
        if (lane >= cnt && lane < S) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ob[lane * 4 + k] = 0.f;
            oi[lane] = -1; os[lane] = 0; on[lane] = 0;
        }
        for (int k = pc + lane; k < A.num_person; k += 64) {
#pragma unroll
            for (int q = 0; q < 4; ++q) op[k * 4 + q] = 0.f;
        }
        if (lane == 0) { A.count[b] = cnt; A.dropped[b] = dropped; A.person_count[b] = pc; }
    }

    // ---- deaths (sort.py:217-219) and the state ----
    {
        const bool live = lane < n && !(t.tsu > A.max_age);
        const unsigned long long lm = __ballot(live);
        const int n_new = popc(lm);
        const int at = popc(lm & below(lane));
        if (live) {
#pragma unroll
            for (int k = 0; k < 7; ++k) sx[k * S + at] = t.x[k];
#pragma unroll
            for (int k = 0; k < 13; ++k) sP[k * S + at] = t.P[k];
            si[at] = t.id; si[S + at] = t.slot; si[2 * S + at] = t.tsu; si[3 * S + at] = t.hits; si[4 * S + at] = t.streak; si[5 * S + at] = t.age;
        }
        if (lane >= n_new && lane < S) {
#pragma unroll
            for (int k = 0; k < 7; ++k) sx[k * S + lane] = 0.0;
#pragma unroll
            for (int k = 0; k < 13; ++k) sP[k * S + lane] = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) si[k * S + lane] = 0;
        }
        if (lane == 0) { hdr[0] = n_new; hdr[1] = next_id; hdr[2] = frame_count; hdr[3] = hold_n; }
    }
}

}  // namespace

int64_t kasf_sort_stream_bytes(int64_t slots, int64_t max_dets) {
    return KASF_SORT_HEADER_BYTES + slots * (20 * 8 + 6 * 4) + max_dets * 16;
}

void kasf_launch_sort_update(hipStream_t s, void* state, int B, int slots, int max_dets, const float* dets, int det_rows, int64_t det_bstride, int64_t det_rstride,
                             const int* det_count, int max_age, int min_hits, float iou_threshold, int num_person, int hold_last, float* boxes, int* ids,
                             int* slot, int* born, int* count, int* dropped, float* persons, int* person_count) {
    TrackArgs a;
    a.state = (unsigned char*)state; a.state_stride = kasf_sort_stream_bytes(slots, max_dets);
    a.dets = dets; a.det_bstride = det_bstride; a.det_rstride = det_rstride; a.det_count = det_count;
    a.boxes = boxes; a.ids = ids; a.slot = slot; a.born = born; a.count = count; a.dropped = dropped; a.persons = persons; a.person_count = person_count;
    a.S = slots; a.D = max_dets; a.R = det_rows; a.max_age = max_age; a.min_hits = min_hits; a.num_person = num_person; a.hold_last = hold_last; a.thr = iou_threshold;
    hipLaunchKernelGGL(k_sort_update, dim3(B), dim3(64), 0, s, a);
}
