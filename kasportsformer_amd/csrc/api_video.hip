// The video chain's C entry points (kasf.h): lift, stream, stream_track, one_euro, coco and world, heatmap, crop, letterbox, yuv, draw, detect, sort.  Each checks its
// arguments (the shared checks are in api_check.h) and calls one launcher of kernels.h.  Every refusal returns before any device call.
#include "api_check.h"

extern "C" {

static const char* lift_plan_error(int64_t n, int32_t T, int32_t stride) {
    if (T < 1 || T > 256) return "lift: T must be in [1, 256]";
    if (stride < 1 || stride > T) return "lift: stride must be in [1, T]";
    if (n < 0) return "lift: n must be >= 0";
    return nullptr;
}
// the plan has a resampled window: the track is shorter than T, or the demo's windows (stride == T) leave a short tail
static bool lift_plan_needs_table(int64_t n, int32_t T, int32_t stride) { return n > 0 && (n < T || (stride == T && n % T != 0)); }

int64_t kasf_lift_window_count(int64_t n, int32_t T, int32_t stride) {
    if (const char* e = lift_plan_error(n, T, stride)) return -(int64_t)kasf_set_error(2, e);
    return kasf_lift_window_count_of(n, T, stride);
}
int kasf_lift_windows(const float* track, int32_t persons, int64_t n, float width, float height, int32_t T, int32_t stride, const int32_t* resample,
                      int32_t flip, float* x_out, void* stream) {
    if (const char* e = lift_plan_error(n, T, stride)) return kasf_set_error(2, e);
    if (persons < 0) return kasf_set_error(2, "lift: persons must be >= 0");
    if (!(width > 0.0f) || !(height > 0.0f)) return kasf_set_error(2, "lift: width and height must be positive");
    if (persons == 0 || n == 0) return 0;
    if (!track || !x_out) return refuse_null();
    if (resample == nullptr && lift_plan_needs_table(n, T, stride)) return kasf_set_error(2, "lift: this plan has a resampled window and needs the resample table");
    kasf_launch_lift_windows((hipStream_t)stream, track, persons, n, width, height, T, stride, resample, flip ? 1 : 0, x_out);
    return api_done();
}
int kasf_lift_stitch(const float* pred, int32_t flip, int32_t persons, int64_t n, int32_t T, int32_t stride, const int32_t* first_pos, float* out,
                     void* stream) {
    if (const char* e = lift_plan_error(n, T, stride)) return kasf_set_error(2, e);
    if (persons < 0) return kasf_set_error(2, "lift: persons must be >= 0");
    if (persons == 0 || n == 0) return 0;
    if (!pred || !out) return refuse_null();
    if (first_pos == nullptr && lift_plan_needs_table(n, T, stride)) return kasf_set_error(2, "lift: this plan has a resampled window and needs first_pos");
    kasf_launch_lift_stitch((hipStream_t)stream, pred, flip ? 1 : 0, persons, n, T, stride, first_pos, out);
    return api_done();
}

int64_t kasf_lift_ragged_plan(const int64_t* lengths, int32_t tracks, int32_t T, int32_t stride, int64_t* win_first) {
    if (const char* e = lift_plan_error(0, T, stride)) return -(int64_t)kasf_set_error(2, e);
    if (tracks < 0) return -(int64_t)kasf_set_error(2, "lift: tracks must be >= 0");
    if (!win_first || (tracks > 0 && !lengths)) return -(int64_t)refuse_null();
    int64_t total = 0;
    for (int32_t p = 0; p < tracks; ++p) {                 // validate everything before writing anything
        if (lengths[p] < 0) return -(int64_t)kasf_set_error(2, "lift: track lengths must be >= 0");
        const int64_t w = kasf_lift_window_count_of(lengths[p], T, stride);
        if (total > INT64_MAX - w) return -(int64_t)kasf_set_error(2, "lift: too many windows");
        total += w;
    }
    win_first[0] = 0;
    for (int32_t p = 0; p < tracks; ++p) win_first[p + 1] = win_first[p] + kasf_lift_window_count_of(lengths[p], T, stride);
    return total;
}
// the host's sizes of the packed arrays: every window has a frame, every frame a track, and no track has more windows than frames
static const char* lift_ragged_error(int32_t tracks, int64_t frames, int64_t windows, int32_t T, int32_t stride) {
    if (const char* e = lift_plan_error(0, T, stride)) return e;
    if (tracks < 0 || frames < 0 || windows < 0) return "lift: tracks, frames and windows must be >= 0";
    if ((frames == 0) != (windows == 0) || windows > frames || (tracks == 0 && frames > 0))
        return "lift: tracks, frames and windows do not belong to one plan";
    return nullptr;
}
int kasf_lift_windows_ragged(const float* packed, const int64_t* offsets, const int64_t* win_first, int32_t tracks, int64_t frames, int64_t windows,
                             const float* width, const float* height, int32_t T, int32_t stride, const int32_t* resample, int32_t flip, float* x_out,
                             void* stream) {
    if (const char* e = lift_ragged_error(tracks, frames, windows, T, stride)) return kasf_set_error(2, e);
    if (windows == 0) return 0;
    if (!packed || !offsets || !win_first || !width || !height || !resample || !x_out) return refuse_null();
    kasf_launch_lift_windows_ragged((hipStream_t)stream, packed, frames, offsets, win_first, tracks, windows, width, height, T, stride, resample,
                                    flip ? 1 : 0, x_out);
    return api_done();
}
int kasf_lift_stitch_ragged(const float* pred, int32_t flip, const int64_t* offsets, const int64_t* win_first, int32_t tracks, int64_t frames,
                            int64_t windows, int32_t T, int32_t stride, const int32_t* first_pos, float* out, void* stream) {
    if (const char* e = lift_ragged_error(tracks, frames, windows, T, stride)) return kasf_set_error(2, e);
    if (frames == 0) return 0;
    if (!pred || !offsets || !win_first || !first_pos || !out) return refuse_null();
    kasf_launch_lift_stitch_ragged((hipStream_t)stream, pred, flip ? 1 : 0, windows, offsets, win_first, tracks, frames, T, stride, first_pos, out);
    return api_done();
}

// ---- one new frame per tick (kasf.h, kasf_stream_*) ----
int kasf_stream_tables(int32_t T, int32_t* resample_tab, int32_t* first_pos_tab) {
    if (T < 1 || T > 256) return kasf_set_error(2, "stream: T must be in [1, 256]");
    if (!resample_tab || !first_pos_tab) return refuse_null();
    for (int64_t i = 0; i < (int64_t)(T + 1) * T; ++i) resample_tab[i] = first_pos_tab[i] = 0;
    for (int32_t n = 1; n <= T; ++n) {
        int32_t* r = resample_tab + (int64_t)n * T;
        int32_t* fp = first_pos_tab + (int64_t)n * T;
        for (int32_t t = 0; t < T; ++t) {                  // demo.py:132-136: np.linspace(0, n, T, endpoint=False) is t * (n / T) in float64; floor; clip
            const int64_t v = (int64_t)floor((double)t * ((double)n / (double)T));
            r[t] = (int32_t)(v < 0 ? 0 : (v > n - 1 ? n - 1 : v));
        }
        for (int32_t t = T - 1; t >= 0; --t) fp[r[t]] = t;  // the first t of every frame (demo.py:146-153, np.unique(r, return_index=True)[1])
    }
    return 0;
}
static const char* stream_error(const void* slots, int32_t K, int32_t S, int32_t T) {
    if (T < 1 || T > 256) return "stream: T must be in [1, 256]";
    if (S < 0 || K < 0 || K > S) return "stream: need 0 <= K <= S";
    if (slots == nullptr && K != 0 && K != S) return "stream: without slot ids the call covers every slot (K == S)";
    return nullptr;
}
int kasf_stream_push(const float* frames, const int32_t* slots, int32_t K, int32_t S, int32_t T, float* ring, int64_t* count, void* stream) {
    if (const char* e = stream_error(slots, K, S, T)) return kasf_set_error(2, e);
    if (K == 0) return 0;
    if (!frames || !ring || !count) return refuse_null();
    kasf_launch_stream_push((hipStream_t)stream, frames, slots, K, S, T, ring, count);
    return api_done();
}
int kasf_stream_windows(const float* ring, const int64_t* count, const int32_t* slots, int32_t K, int32_t S, int32_t T, const float* width,
                        const float* height, const int32_t* resample_tab, int32_t flip, float* x_out, void* stream) {
    if (const char* e = stream_error(slots, K, S, T)) return kasf_set_error(2, e);
    if (K == 0) return 0;
    if (!ring || !count || !width || !height || !resample_tab || !x_out) return refuse_null();
    kasf_launch_stream_windows((hipStream_t)stream, ring, count, slots, K, S, T, width, height, resample_tab, flip ? 1 : 0, x_out);
    return api_done();
}
int kasf_stream_emit(const float* pred, int32_t flip, const int64_t* count, const int32_t* slots, int32_t K, int32_t S, int32_t T,
                     const int32_t* first_pos_tab, int32_t back, int32_t n_out, float* out, void* stream) {
    if (const char* e = stream_error(slots, K, S, T)) return kasf_set_error(2, e);
    if (back < 0 || back > T - 1) return kasf_set_error(2, "stream: back must be in [0, T - 1]");
    if (n_out < 0 || n_out > T) return kasf_set_error(2, "stream: n_out must be in [0, T]");
    if (K == 0 || n_out == 0) return 0;
    if (!pred || !count || !first_pos_tab || !out) return refuse_null();
    kasf_launch_stream_emit((hipStream_t)stream, pred, flip ? 1 : 0, count, slots, K, S, T, first_pos_tab, back, n_out, out);
    return api_done();
}

// ---- the stream lifter's slots driven by the tracker's output (kasf.h, kasf_stream_track_*) ----
int kasf_stream_track_front(const float* frames, const int32_t* ids, const int32_t* slot, const int32_t* born, const int32_t* count_b, int32_t streams,
                            int32_t track_slots, int32_t rows_mode, int32_t R, int32_t T, float* ring, int64_t* count, int32_t* owner, const float* width,
                            const float* height, const int32_t* resample_tab, int32_t flip, float* x_out, int32_t* row_slot, void* stream) {
    if (T < 1 || T > 256) return kasf_set_error(2, "stream_track: T must be in [1, 256]");
    if (refuse_tracked_rows("stream_track", streams, track_slots, rows_mode, R)) return 2;
    if (!frames || !ids || !slot || !born || !count_b || !ring || !count || !owner || !width || !height || !resample_tab || !x_out || !row_slot)
        return refuse_null();
    kasf_launch_stream_track_front((hipStream_t)stream, frames, ids, slot, born, count_b, streams, track_slots, rows_mode, R, T, ring, count, owner, width, height,
                                   resample_tab, flip ? 1 : 0, x_out, row_slot);
    return api_done();
}
int kasf_stream_track_emit(const float* pred, int32_t flip, const int64_t* count, const int32_t* owner, const int32_t* row_slot, int32_t n_rows, int32_t T,
                           const int32_t* first_pos_tab, int32_t back, float* out, uint8_t* valid, int32_t* ids_out, int64_t* frames_out, void* stream) {
    if (T < 1 || T > 256) return kasf_set_error(2, "stream_track: T must be in [1, 256]");
    if (back < 0 || back > T - 1) return kasf_set_error(2, "stream_track: back must be in [0, T - 1]");
    if (n_rows < 0) return kasf_set_error(2, "stream_track: n_rows must be >= 0");
    if (n_rows == 0) return 0;
    if (!pred || !count || !owner || !row_slot || !first_pos_tab || !out || !valid || !ids_out || !frames_out) return refuse_null();
    kasf_launch_stream_track_emit((hipStream_t)stream, pred, flip ? 1 : 0, count, owner, row_slot, n_rows, T, first_pos_tab, back, out, valid, ids_out, frames_out);
    return api_done();
}

// ---- the One-Euro filter with its state on the device (kasf.h, kasf_one_euro_*) ----
static const char* one_euro_error(int32_t J, int32_t C, const kasf_one_euro_params* p, KasfOneEuro* out) {
    if (J < 1 || J > 256) return "one_euro: J must be in [1, 256]";
    if (C < 1 || C > 4) return "one_euro: C must be in [1, 4]";
    if (p == nullptr) return "null pointer argument";
    const float in_hz[3] = {p->dt, p->min_cutoff, p->d_cutoff};
    for (float v : in_hz)
        if (!(v >= 1e-6f && v <= 1e6f)) return "one_euro: dt, min_cutoff and d_cutoff must be in [1e-6, 1e6]";
    if (!(p->beta >= 0.0f && p->beta <= 1e6f)) return "one_euro: beta must be in [0, 1e6]";
    if (!std::isfinite(p->min_score)) return "one_euro: min_score must be finite";
    if (p->max_hold < 0 || p->max_hold > (1 << 20)) return "one_euro: max_hold must be in [0, 2^20]";
    *out = KasfOneEuro{p->dt, p->min_cutoff, p->d_cutoff, p->beta, p->min_score, p->max_hold};
    return nullptr;
}
int kasf_one_euro_push(const float* x, const int32_t* slots, int32_t K, int32_t S, int32_t J, int32_t C, int32_t has_score, const kasf_one_euro_params* params,
                       int64_t tick, float* xhat, float* dxhat, int64_t* last, float* out, void* stream) {
    KasfOneEuro p;
    if (const char* e = one_euro_error(J, C, params, &p)) return kasf_set_error(2, e);
    if (const char* e = stream_error(slots, K, S, 1)) return kasf_set_error(2, e);
    if (tick < 0) return kasf_set_error(2, "one_euro: tick must be >= 0");
    if (K == 0) return 0;
    if (!x || !xhat || !dxhat || !last || !out) return refuse_null();
    kasf_launch_one_euro_push((hipStream_t)stream, x, slots, K, S, J, C, has_score ? 1 : 0, p, tick, xhat, dxhat, last, out);
    return api_done();
}
int kasf_one_euro_tracked(const float* x, const int32_t* ids, const int32_t* slot, const int32_t* born, const int32_t* count_b, int32_t streams,
                          int32_t track_slots, int32_t rows_mode, int32_t R, int32_t J, int32_t C, int32_t has_score, const kasf_one_euro_params* params,
                          int64_t tick, float* xhat, float* dxhat, int64_t* last, int32_t* owner, float* out, int32_t* row_slot, void* stream) {
    KasfOneEuro p;
    if (const char* e = one_euro_error(J, C, params, &p)) return kasf_set_error(2, e);
    if (refuse_tracked_rows("one_euro", streams, track_slots, rows_mode, R)) return 2;
    if (tick < 0) return kasf_set_error(2, "one_euro: tick must be >= 0");
    if (!x || !ids || !slot || !born || !count_b || !xhat || !dxhat || !last || !owner || !out) return refuse_null();
    kasf_launch_one_euro_tracked((hipStream_t)stream, x, ids, slot, born, count_b, streams, track_slots, rows_mode, R, J, C, has_score ? 1 : 0, p, tick, xhat, dxhat,
                                 last, owner, out, row_slot);
    return api_done();
}
int kasf_one_euro_tracks(const float* x, const int64_t* offsets, int64_t N, int32_t P, int32_t J, int32_t C, int32_t has_score,
                         const kasf_one_euro_params* params, float* out, void* stream) {
    KasfOneEuro p;
    if (const char* e = one_euro_error(J, C, params, &p)) return kasf_set_error(2, e);
    if (P < 0 || N < 0) return kasf_set_error(2, "one_euro: P and N must be >= 0");
    if (P == 0) return 0;
    if (!offsets || (N > 0 && (!x || !out))) return refuse_null();
    kasf_launch_one_euro_tracks((hipStream_t)stream, x, offsets, N, P, J, C, has_score ? 1 : 0, p, out);
    return api_done();
}

// ---- the two ends of the lift (kasf.h, kasf_coco_h36m / kasf_pose_world) ----
int kasf_coco_h36m(const float* coco, int64_t frames, float* h36m, void* stream) {
    if (frames < 0) return kasf_set_error(2, "coco_h36m: frames must be >= 0");
    if (frames == 0) return 0;
    if (!coco || !h36m) return refuse_null();
    kasf_launch_coco_h36m((hipStream_t)stream, coco, frames, h36m);
    return api_done();
}
int kasf_pose_world(const float* poses, int64_t frames, const float* quat4, const float* trans3, int32_t floor, int32_t unit, float* out, void* stream) {
    if (frames < 0) return kasf_set_error(2, "pose_world: frames must be >= 0");
    if (frames == 0) return 0;
    if (!poses || !quat4 || !out) return refuse_null();
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    kasf_launch_pose_world((hipStream_t)stream, poses, frames, quat4, trans3 ? trans3 : zero, floor ? 1 : 0, unit ? 1 : 0, out);
    return api_done();
}

// ---- pose-network heatmaps -> keypoints (kasf.h, kasf_heatmap_keypoints) ----
// what the plain and the flip-tested entry point refuse alike, in this order; who = the entry point's name in its messages
static int heatmap_refusal(const char* who, int64_t n, int32_t H, int32_t W, int32_t dtype, int32_t geom_kind, int32_t out_layout, double aspect) {
    if (n < 0) return refuse(who, "n must be >= 0");
    if (H < 1 || W < 1) return refuse(who, "H and W must be >= 1");
    if ((int64_t)H * W > ((int64_t)1 << 24)) return refuse(who, "H * W must be <= 2^24 (the reference's index arithmetic is fp32)");
    if (refuse_dtype3(who, "dtype", dtype)) return 2;
    if (geom_kind != KASF_GEOM_CENTER_SCALE && geom_kind != KASF_GEOM_BOX) return refuse(who, "geom_kind must be KASF_GEOM_CENTER_SCALE or KASF_GEOM_BOX");
    if (out_layout != KASF_LAYOUT_COCO && out_layout != KASF_LAYOUT_H36M) return refuse(who, "out_layout must be KASF_LAYOUT_COCO or KASF_LAYOUT_H36M");
    return geom_kind == KASF_GEOM_BOX && !(aspect > 0.0) ? refuse(who, "aspect must be > 0 with KASF_GEOM_BOX") : 0;
}
int kasf_heatmap_keypoints(const void* hm, int32_t dtype, int64_t n, int32_t H, int32_t W, const float* geom, int32_t geom_kind, double aspect, int32_t refine,
                           int32_t out_layout, float* out, float* coco_scratch, void* stream) {
    if (heatmap_refusal("heatmap_keypoints", n, H, W, dtype, geom_kind, out_layout, aspect)) return 2;
    if (n == 0) return 0;
    if (!hm || !geom || !out || (out_layout == KASF_LAYOUT_H36M && !coco_scratch)) return refuse_null();
    const bool h36m = out_layout == KASF_LAYOUT_H36M;
    kasf_launch_heatmap_keypoints((hipStream_t)stream, hm, dtype, n, H, W, geom, geom_kind, aspect, refine ? 1 : 0, h36m ? coco_scratch : out);
    if (h36m) kasf_launch_coco_h36m((hipStream_t)stream, coco_scratch, n, out);
    return api_done();
}

// ---- flip-tested pose-network heatmaps -> keypoints (kasf.h, kasf_heatmap_flip_keypoints) ----
int kasf_heatmap_flip_keypoints(const void* hm, const void* hm_flipped, int32_t dtype, int64_t n, int32_t H, int32_t W, const int32_t* partner, int32_t shift,
                                const float* geom, int32_t geom_kind, double aspect, int32_t refine, int32_t out_layout, float* out, float* coco_scratch,
                                float* merged_out, void* stream) {
    if (heatmap_refusal("heatmap_flip_keypoints", n, H, W, dtype, geom_kind, out_layout, aspect)) return 2;
    const int32_t* pt = partner_or_coco(partner);
    if (refuse_partner("heatmap_flip_keypoints", pt)) return 2;
    if (n == 0) return 0;
    if (!hm || !hm_flipped || !geom || !out || (out_layout == KASF_LAYOUT_H36M && !coco_scratch)) return refuse_null();
    if (merged_out && ((const void*)merged_out == hm || (const void*)merged_out == hm_flipped))
        return kasf_set_error(2, "heatmap_flip_keypoints: merged_out must not overlap hm or hm_flipped");
    const bool h36m = out_layout == KASF_LAYOUT_H36M;
    int pv[17];
    for (int j = 0; j < 17; ++j) pv[j] = pt[j];
    kasf_launch_heatmap_flip_keypoints((hipStream_t)stream, hm, hm_flipped, dtype, n, H, W, pv, shift ? 1 : 0, geom, geom_kind, aspect, refine ? 1 : 0,
                                       h36m ? coco_scratch : out, merged_out);
    if (h36m) kasf_launch_coco_h36m((hipStream_t)stream, coco_scratch, n, out);
    return api_done();
}

// ---- DARK / UDP sub-pixel heatmap decode (kasf.h, kasf_heatmap_decode) ----
int kasf_heatmap_decode(const void* hm, const void* hm_flipped, int32_t dtype, int64_t n, int32_t H, int32_t W, const int32_t* partner, int32_t shift,
                        const float* geom, int32_t geom_kind, double aspect, int32_t mode, const float* weights, int32_t K, int32_t udp, int32_t out_layout,
                        float* out, float* coco_scratch, float* merged_out, void* stream) {
    if (heatmap_refusal("heatmap_decode", n, H, W, dtype, geom_kind, out_layout, aspect)) return 2;
    if (mode != KASF_DECODE_QUARTER && mode != KASF_DECODE_DARK && mode != KASF_DECODE_DARK_UDP)
        return kasf_set_error(2, "heatmap_decode: mode must be KASF_DECODE_QUARTER, _DARK or _DARK_UDP");
    if (K < 1 || K > 17 || K % 2 == 0) return kasf_set_error(2, "heatmap_decode: K must be odd and in [1, 17]");
    if (mode != KASF_DECODE_QUARTER && !weights) return kasf_set_error(2, "heatmap_decode: weights must be given with KASF_DECODE_DARK and _DARK_UDP");
    if (udp && (H < 2 || W < 2)) return kasf_set_error(2, "heatmap_decode: udp needs H and W >= 2");
    const int32_t* pt = partner_or_coco(partner);
    if ((hm_flipped || partner) && refuse_partner("heatmap_decode", pt)) return 2;
    if (n == 0) return 0;
    if (!hm || !geom || !out || (out_layout == KASF_LAYOUT_H36M && !coco_scratch)) return refuse_null();
    if (merged_out && !hm_flipped) return kasf_set_error(2, "heatmap_decode: merged_out goes with hm_flipped");
    if (merged_out && ((const void*)merged_out == hm || (const void*)merged_out == hm_flipped))
        return kasf_set_error(2, "heatmap_decode: merged_out must not overlap hm or hm_flipped");
    const bool h36m = out_layout == KASF_LAYOUT_H36M;
    int pv[17];
    for (int j = 0; j < 17; ++j) pv[j] = pt[j];
    kasf_launch_heatmap_decode((hipStream_t)stream, hm, hm_flipped, dtype, n, H, W, pv, shift ? 1 : 0, geom, geom_kind, aspect, mode, weights, K, udp ? 1 : 0,
                               h36m ? coco_scratch : out, merged_out);
    if (h36m) kasf_launch_coco_h36m((hipStream_t)stream, coco_scratch, n, out);
    return api_done();
}

// ---- person boxes -> pose-network inputs (kasf.h, kasf_crop_persons) ----
int kasf_crop_persons(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride, const int32_t* frame_index,
                      const float* geom, int32_t geom_kind, double aspect, int64_t n, void* out, int32_t out_dtype, int32_t out_w, int32_t out_h,
                      const float* mean_std, int32_t swap_rb, float* center_scale_out, void* stream) {
    if (n < 0) return kasf_set_error(2, "crop_persons: n must be >= 0");
    if (out_w < 1 || out_h < 1 || out_w > 32767 || out_h > 32767) return kasf_set_error(2, "crop_persons: out_w and out_h must be in [1, 32767]");
    if (refuse_frame_size("crop_persons", Hf, Wf)) return 2;
    if (n_frames < 1) return kasf_set_error(2, "crop_persons: n_frames must be >= 1");
    if (refuse_row_stride("crop_persons", "row", row_stride, Wf)) return 2;
    if (n_frames > 1 && frame_stride < 0) return kasf_set_error(2, "crop_persons: the frame stride must be >= 0");
    if (refuse_dtype3("crop_persons", "out_dtype", out_dtype)) return 2;
    if (geom_kind != KASF_GEOM_CENTER_SCALE && geom_kind != KASF_GEOM_BOX) return kasf_set_error(2, "crop_persons: geom_kind must be KASF_GEOM_CENTER_SCALE or KASF_GEOM_BOX");
    if (geom_kind == KASF_GEOM_BOX && !(aspect > 0.0)) return kasf_set_error(2, "crop_persons: aspect must be > 0 with KASF_GEOM_BOX");
    if (!mean_std) return refuse_null();
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(mean_std[3 + c]) || mean_std[3 + c] == 0.0f) return kasf_set_error(2, "crop_persons: every std must be finite and not 0");
    if (n == 0) return 0;
    if (!frames || !geom || !out || (n_frames > 1 && !frame_index)) return refuse_null();
    kasf_launch_crop_persons((hipStream_t)stream, frames, n_frames, Hf, Wf, row_stride, frame_stride, frame_index, geom, geom_kind, aspect, n, out, out_dtype,
                             out_w, out_h, mean_std, swap_rb ? 1 : 0, center_scale_out);
    return api_done();
}

// ---- video frames -> detector inputs (kasf.h, kasf_letterbox_plan / kasf_letterbox_frames) ----
int kasf_letterbox_plan(int32_t Wf, int32_t Hf, int32_t out_w, int32_t out_h, int32_t* new_w, int32_t* new_h, int32_t* pad_x, int32_t* pad_y) {
    if (refuse_frame_size("letterbox", Hf, Wf)) return 2;
    if (out_w < 1 || out_h < 1 || out_w > KASF_LETTERBOX_MAX_SIDE || out_h > KASF_LETTERBOX_MAX_SIDE)
        return kasf_set_error(2, "letterbox: out_w and out_h must be in [1, 4096] (KASF_LETTERBOX_MAX_SIDE: one table entry per output column in LDS)");
    if (!new_w || !new_h || !pad_x || !pad_y) return refuse_null();
    // rule 1: the reference's int(img_w * min(w / img_w, h / img_h)) in the same IEEE doubles
    const double rw = (double)out_w / (double)Wf, rh = (double)out_h / (double)Hf;
    const double r = rh < rw ? rh : rw;
    const int32_t nw = (int32_t)((double)Wf * r), nh = (int32_t)((double)Hf * r);
    if (nw < 1 || nh < 1) return kasf_set_error(2, "letterbox: the frame is so elongated that the resized image has no pixels (new_w or new_h < 1)");
    *new_w = nw; *new_h = nh;
    *pad_x = (out_w - nw) / 2; *pad_y = (out_h - nh) / 2;
    return 0;
}

int kasf_letterbox_frames(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride, void* out, int32_t out_dtype,
                          int32_t out_w, int32_t out_h, int32_t pad_value, int32_t swap_rb, void* stream) {
    if (n_frames < 0) return kasf_set_error(2, "letterbox_frames: n_frames must be >= 0");
    int32_t new_w, new_h, pad_x, pad_y;
    if (kasf_letterbox_plan(Wf, Hf, out_w, out_h, &new_w, &new_h, &pad_x, &pad_y)) return 2;
    if (refuse_row_stride("letterbox_frames", "row", row_stride, Wf)) return 2;
    if (frame_stride < 0) return kasf_set_error(2, "letterbox_frames: the frame stride must be >= 0");
    if (plane_uncovered(n_frames, frame_stride, Hf, row_stride))
        return kasf_set_error(2, "letterbox_frames: the frame stride must be at least Hf * row_stride with more than one frame");
    if (refuse_dtype3("letterbox_frames", "out_dtype", out_dtype)) return 2;
    if (pad_value < 0 || pad_value > 255) return kasf_set_error(2, "letterbox_frames: pad_value must be in [0, 255]");
    if (n_frames == 0) return 0;
    if (!frames || !out) return refuse_null();
    kasf_launch_letterbox((hipStream_t)stream, frames, n_frames, Hf, Wf, row_stride, frame_stride, out, out_dtype, out_w, out_h, new_w, new_h, pad_x, pad_y,
                          pad_value, swap_rb ? 1 : 0);
    return api_done();
}

// ---- decoder surfaces -> BGR frames (kasf.h, kasf_yuv420_to_bgr) ----
int kasf_yuv420_to_bgr(const void* y, const void* c0, const void* c1, int32_t layout, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t y_row_stride,
                       int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride, void* out, int64_t out_row_stride, int64_t out_frame_stride,
                       int32_t matrix, int32_t full_range, int32_t rgb, void* stream) {
    const char* const who = "yuv420_to_bgr";
    static const int kCoef[2][2][5] = {{KASF_YUV_COEF_BT601_LIMITED, KASF_YUV_COEF_BT601_FULL}, {KASF_YUV_COEF_BT709_LIMITED, KASF_YUV_COEF_BT709_FULL}};
    if (n_frames < 0) return kasf_set_error(2, "yuv420_to_bgr: n_frames must be >= 0");
    if (refuse_frame_size(who, Hf, Wf)) return 2;
    if (layout != KASF_YUV_NV12 && layout != KASF_YUV_I420) return kasf_set_error(2, "yuv420_to_bgr: layout must be KASF_YUV_NV12 or KASF_YUV_I420");
    if (matrix != KASF_YUV_BT601 && matrix != KASF_YUV_BT709) return kasf_set_error(2, "yuv420_to_bgr: matrix must be KASF_YUV_BT601 or KASF_YUV_BT709");
    const bool nv12 = layout == KASF_YUV_NV12;
    const int64_t cw = (Wf + 1) / 2, ch = (Hf + 1) / 2;
    if (refuse_yuv_rows(who, y_row_stride, c_row_stride, Wf, nv12 ? 2 * cw : cw, "2 * ((Wf + 1) / 2) bytes for NV12, (Wf + 1) / 2 for I420")) return 2;
    if (refuse_row_stride(who, "output row", out_row_stride, Wf)) return 2;
    if (y_frame_stride < 0 || c_frame_stride < 0 || out_frame_stride < 0) return kasf_set_error(2, "yuv420_to_bgr: the frame strides must be >= 0");
    if (refuse_plane(who, n_frames, y_frame_stride, Hf, y_row_stride) || refuse_plane(who, n_frames, c_frame_stride, ch, c_row_stride) ||
        refuse_plane(who, n_frames, out_frame_stride, Hf, out_row_stride))
        return 2;
    if (nv12 ? c1 != nullptr : c1 == nullptr) return kasf_set_error(2, "yuv420_to_bgr: c1 is the V plane of I420 and must be NULL for NV12");
    if (n_frames == 0) return 0;
    if (!y || !c0 || !out) return refuse_null();
    kasf_launch_yuv420_to_bgr((hipStream_t)stream, y, c0, c1, nv12 ? 1 : 0, n_frames, Hf, Wf, y_row_stride, c_row_stride, y_frame_stride, c_frame_stride, out,
                              out_row_stride, out_frame_stride, kCoef[matrix][full_range ? 1 : 0], full_range ? 1 : 0, rgb ? 1 : 0);
    return api_done();
}

// ---- skeletons over the frame and the encoder's surface (kasf.h, kasf_draw_poses / kasf_bgr_to_nv12 / kasf_pose_panel) ----
int kasf_draw_poses(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride, const float* keypoints, int32_t P,
                    int32_t J, int32_t C, int64_t kp_frame_stride, int64_t kp_person_stride, int64_t kp_joint_stride, int64_t kp_coord_stride,
                    const uint8_t* valid, int64_t valid_frame_stride, int64_t valid_person_stride, const int32_t* segments, const uint8_t* colors, int32_t S,
                    const uint8_t* dot_color, int32_t thickness, int32_t dot_radius, float min_score, const int32_t* fills, int32_t R, void* out_bgr,
                    int64_t out_row_stride, int64_t out_frame_stride, void* out_y, void* out_uv, int64_t y_row_stride, int64_t uv_row_stride,
                    int64_t y_frame_stride, int64_t uv_frame_stride, int32_t matrix, int32_t full_range, int32_t rgb, void* stream) {
    const char* const who = "draw_poses";
    static const int kCoef[2][2][8] = {{KASF_RGB2YUV_COEF_BT601_LIMITED, KASF_RGB2YUV_COEF_BT601_FULL}, {KASF_RGB2YUV_COEF_BT709_LIMITED, KASF_RGB2YUV_COEF_BT709_FULL}};
    if (n_frames < 0) return kasf_set_error(2, "draw_poses: n_frames must be >= 0");
    if (refuse_frame_size(who, Hf, Wf)) return 2;
    if (matrix != KASF_YUV_BT601 && matrix != KASF_YUV_BT709) return kasf_set_error(2, "draw_poses: matrix must be KASF_YUV_BT601 or KASF_YUV_BT709");
    if (!out_bgr && !out_y && !out_uv) return kasf_set_error(2, "draw_poses: out_bgr, or out_y and out_uv, must be given");
    if (!out_y != !out_uv) return kasf_set_error(2, "draw_poses: out_y and out_uv are one surface: both or neither");
    const int64_t cw = (Wf + 1) / 2, ch = (Hf + 1) / 2;
    if (refuse_row_stride(who, "row", row_stride, Wf)) return 2;
    if (frame_stride < 0) return kasf_set_error(2, "draw_poses: the frame strides must be >= 0");
    if (refuse_plane(who, n_frames, frame_stride, Hf, row_stride)) return 2;
    if (out_bgr) {
        if (refuse_row_stride(who, "output row", out_row_stride, Wf)) return 2;
        if (out_frame_stride < 0) return kasf_set_error(2, "draw_poses: the frame strides must be >= 0");
        if (refuse_plane(who, n_frames, out_frame_stride, Hf, out_row_stride)) return 2;
    }
    if (out_y) {
        if (refuse_yuv_rows(who, y_row_stride, uv_row_stride, Wf, 2 * cw, "2 * ((Wf + 1) / 2) bytes")) return 2;
        if (y_frame_stride < 0 || uv_frame_stride < 0) return kasf_set_error(2, "draw_poses: the frame strides must be >= 0");
        if (refuse_plane(who, n_frames, y_frame_stride, Hf, y_row_stride) || refuse_plane(who, n_frames, uv_frame_stride, ch, uv_row_stride)) return 2;
    }
    if (P < 0 || P > (1 << 20)) return kasf_set_error(2, "draw_poses: P must be in [0, 2^20]");
    if (S < 0 || S > 32) return kasf_set_error(2, "draw_poses: S must be in [0, 32]");
    if (P > 0 && S > 0) {
        if (J < 1 || J > 32) return kasf_set_error(2, "draw_poses: J must be in [1, 32]");
        if (C != 2 && C != 3) return kasf_set_error(2, "draw_poses: C must be 2 (x, y) or 3 (x, y, score)");
        if (!keypoints || !segments || !colors) return refuse_null();
    }
    if (!dot_color) return refuse_null();
    if (thickness < 1 || thickness > 64) return kasf_set_error(2, "draw_poses: thickness must be in [1, 64]");
    if (dot_radius < 0 || dot_radius > 32) return kasf_set_error(2, "draw_poses: dot_radius must be in [0, 32]");
    if (R < 0 || R > 8) return kasf_set_error(2, "draw_poses: R must be in [0, 8]");
    if (R > 0 && !fills) return refuse_null();
    if (n_frames == 0) return 0;
    if (!frames) return refuse_null();
    KasfDrawLaunch d;
    d.frames = frames; d.n_frames = n_frames; d.Hf = Hf; d.Wf = Wf; d.row_stride = row_stride; d.frame_stride = frame_stride;
    d.keypoints = keypoints; d.P = P; d.J = J; d.use_score = (C == 3 && std::isfinite(min_score)) ? 1 : 0;
    d.kp_frame_stride = kp_frame_stride; d.kp_person_stride = kp_person_stride; d.kp_joint_stride = kp_joint_stride; d.kp_coord_stride = kp_coord_stride;
    d.valid = valid; d.valid_frame_stride = valid_frame_stride; d.valid_person_stride = valid_person_stride;
    d.segments = segments; d.colors = colors; d.S = S;
    for (int c = 0; c < 3; ++c) d.dot_color[c] = dot_color[c];
    d.thickness = thickness; d.dot_radius = dot_radius; d.min_score = min_score; d.fills = fills; d.R = R;
    d.out_bgr = out_bgr; d.out_row_stride = out_row_stride; d.out_frame_stride = out_frame_stride;
    d.out_y = out_y; d.out_uv = out_uv; d.y_row_stride = y_row_stride; d.uv_row_stride = uv_row_stride; d.y_frame_stride = y_frame_stride;
    d.uv_frame_stride = uv_frame_stride;
    d.coef = kCoef[matrix][full_range ? 1 : 0]; d.full_range = full_range ? 1 : 0; d.rgb = rgb ? 1 : 0;
    kasf_launch_draw_poses((hipStream_t)stream, &d);
    return api_done();
}

int kasf_bgr_to_nv12(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride, void* out_y, void* out_uv,
                     int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride, int64_t uv_frame_stride, int32_t matrix, int32_t full_range, int32_t rgb,
                     void* stream) {
    static const uint8_t kNoDot[3] = {0, 0, 0};
    if (!out_y || !out_uv) return refuse_null();
    return kasf_draw_poses(frames, n_frames, Hf, Wf, row_stride, frame_stride, nullptr, 0, 0, 0, 0, 0, 0, 0, nullptr, 0, 0, nullptr, nullptr, 0, kNoDot, 1, 0, 0.0f,
                           nullptr, 0, nullptr, 0, 0, out_y, out_uv, y_row_stride, uv_row_stride, y_frame_stride, uv_frame_stride, matrix, full_range, rgb, stream);
}

int kasf_pose_panel(const float* poses, int64_t n, const float* view, float* out, void* stream) {
    if (n < 0 || n > ((int64_t)1 << 40)) return kasf_set_error(2, "pose_panel: n must be in [0, 2^40]");
    if (!view) return refuse_null();
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(view[i])) return kasf_set_error(2, "pose_panel: every view coefficient must be finite");
    if (n == 0) return 0;
    if (!poses || !out) return refuse_null();
    kasf_launch_pose_panel((hipStream_t)stream, poses, n, view, out);
    return api_done();
}

// ---- detector output -> person boxes (kasf.h, kasf_detect_boxes) ----
static const char* detect_shape_error(int32_t batch, int64_t n_per_image, int32_t max_candidates) {
    if (batch < 0 || batch > 65535) return "detect: batch must be in [0, 65535]";
    if (n_per_image < 1 || n_per_image > ((int64_t)1 << 24)) return "detect: candidates per image must be in [1, 2^24]";
    if (max_candidates < 1 || max_candidates > KASF_DETECT_MAX_CANDIDATES) return "detect: max_candidates must be in [1, 4096] (KASF_DETECT_MAX_CANDIDATES: sort and NMS run in LDS)";
    return nullptr;
}
int64_t kasf_detect_workspace_bytes(int32_t batch, int64_t n_per_image, int32_t max_candidates) {
    if (const char* e = detect_shape_error(batch, n_per_image, max_candidates)) return -(int64_t)kasf_set_error(2, e);
    return kasf_detect_ws_bytes(batch, n_per_image);
}
int kasf_detect_boxes(const void* const* src, int32_t n_src, int32_t form, int32_t dtype, int32_t batch, const int32_t* grid, int32_t A, int32_t C,
                      const float* anchors, int32_t inp_dim, const float* frame_wh, float confidence, float nms, int32_t class_id, int32_t max_candidates,
                      int32_t max_boxes, float* boxes, int32_t* index, int32_t* count, void* workspace, int64_t workspace_bytes, void* stream) {
    if (form != KASF_DETECT_PREDICTION && form != KASF_DETECT_HEADS) return kasf_set_error(2, "detect_boxes: form must be KASF_DETECT_PREDICTION or KASF_DETECT_HEADS");
    if (refuse_dtype3("detect_boxes", "dtype", dtype)) return 2;
    if (n_src < 1 || n_src > KASF_DETECT_MAX_SRC || (form == KASF_DETECT_PREDICTION && n_src != 1))
        return kasf_set_error(2, "detect_boxes: n_src must be in [1, 4], and 1 in the prediction form");
    if (!src || !grid) return refuse_null();
    if (C < 1 || C > 65536) return kasf_set_error(2, "detect_boxes: C must be in [1, 65536]");
    if (class_id < 0 || class_id >= C) return kasf_set_error(2, "detect_boxes: class_id must be in [0, C)");
    if (inp_dim < 1) return kasf_set_error(2, "detect_boxes: inp_dim must be >= 1");
    int64_t N = 0;
    if (form == KASF_DETECT_HEADS) {
        if (A < 1 || A > KASF_DETECT_MAX_A) return kasf_set_error(2, "detect_boxes: A must be in [1, 8]");
        if (!anchors) return refuse_null();
        for (int k = 0; k < n_src; ++k) {
            if (grid[k] < 1 || grid[k] > 4096 || inp_dim % grid[k] != 0) return kasf_set_error(2, "detect_boxes: every grid must be in [1, 4096] and divide inp_dim");
            N += (int64_t)grid[k] * grid[k] * A;
        }
    } else {
        N = grid[0];
    }
    if (const char* e = detect_shape_error(batch, N, max_candidates)) return kasf_set_error(2, e);
    if (max_boxes < 1 || max_boxes > max_candidates) return kasf_set_error(2, "detect_boxes: max_boxes must be in [1, max_candidates]");
    if (!std::isfinite(confidence) || !std::isfinite(nms)) return kasf_set_error(2, "detect_boxes: confidence and nms must be finite");
    if (batch == 0) return 0;
    for (int k = 0; k < n_src; ++k)
        if (!src[k]) return refuse_null();
    if (!frame_wh || !boxes || !index || !count || !workspace) return refuse_null();
    if (misaligned16(workspace)) return kasf_set_error(2, "detect_boxes: workspace must be 16-byte aligned");
    if (workspace_bytes < kasf_detect_ws_bytes(batch, N)) return kasf_set_error(2, "detect_boxes: workspace too small (see kasf_detect_workspace_bytes)");
    if (const char* e = kasf_launch_detect_boxes((hipStream_t)stream, src, n_src, form, dtype, batch, grid, A, C, anchors, inp_dim, frame_wh, confidence, nms,
                                                 class_id, max_candidates, max_boxes, boxes, index, count, workspace))
        return kasf_set_error(3, e);
    return api_done();
}

// ---- person boxes -> tracked person boxes (kasf.h, kasf_sort_update) ----
static const char* sort_shape_error(int32_t streams, int32_t slots, int32_t max_dets) {
    if (streams < 0 || streams > 65535) return "sort: streams must be in [0, 65535]";
    if (slots < 1 || slots > KASF_SORT_MAX) return "sort: slots must be in [1, 64] (one lane of a wavefront per track)";
    if (max_dets < 1 || max_dets > KASF_SORT_MAX) return "sort: max_dets must be in [1, 64] (one lane of a wavefront per detection)";
    return nullptr;
}
int64_t kasf_sort_state_bytes(int32_t streams, int32_t slots, int32_t max_dets) {
    if (const char* e = sort_shape_error(streams, slots, max_dets)) return -(int64_t)kasf_set_error(2, e);
    return (int64_t)streams * kasf_sort_stream_bytes(slots, max_dets);
}
int kasf_sort_update(void* state, int32_t streams, int32_t slots, int32_t max_dets, const float* dets, int32_t det_rows, int64_t det_stream_stride, int64_t det_row_stride,
                     const int32_t* det_count, int32_t max_age, int32_t min_hits, float iou_threshold, int32_t num_person, int32_t hold_last, float* boxes,
                     int32_t* ids, int32_t* slot, int32_t* born, int32_t* count, int32_t* dropped, float* persons, int32_t* person_count, void* stream) {
    if (const char* e = sort_shape_error(streams, slots, max_dets)) return kasf_set_error(2, e);
    if (det_rows < 0 || det_rows > max_dets) return kasf_set_error(2, "sort_update: det_rows must be in [0, max_dets]");
    if (det_row_stride < 4) return kasf_set_error(2, "sort_update: the detection row stride must be at least 4 elements");
    if (det_stream_stride < 0) return kasf_set_error(2, "sort_update: the detection stream stride must be >= 0");
    if (max_age < 0 || min_hits < 0) return kasf_set_error(2, "sort_update: max_age and min_hits must be >= 0");
    if (!std::isfinite(iou_threshold)) return kasf_set_error(2, "sort_update: iou_threshold must be finite");
    if (num_person < 1 || num_person > 65535) return kasf_set_error(2, "sort_update: num_person must be in [1, 65535]");
    if (streams == 0) return 0;
    if (!state || (!dets && det_rows > 0) || !boxes || !ids || !slot || !born || !count || !dropped || !persons || !person_count) return refuse_null();
    if (((uintptr_t)state & 7) != 0) return kasf_set_error(2, "sort_update: state must be 8-byte aligned");
    kasf_launch_sort_update((hipStream_t)stream, state, streams, slots, max_dets, dets, det_rows, det_stream_stride, det_row_stride, det_count, max_age, min_hits,
                            iou_threshold, num_person, hold_last ? 1 : 0, boxes, ids, slot, born, count, dropped, persons, person_count);
    return api_done();
}

}  // extern "C"
