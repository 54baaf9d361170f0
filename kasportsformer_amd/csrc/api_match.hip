// The C entry points of the cross-camera matching (kasf.h, kasf_match_workspace_bytes / kasf_match_pair_costs / kasf_match_groups), built like
// api_triangulate.hip: they check their arguments before a device or a device pointer is touched, with api_check.h's refusals, and launch k_match.hip's kernels
// (tests/test_match_refusals_cpu.py holds every message here to a case).
#include "api_check.h"
#include "camera_model.h"

namespace {

int refuse_match_shape(const char* who, int32_t cameras, int32_t rows, int64_t frames) {
    if (cameras < 2 || cameras > KASF_MATCH_MAX_CAMERAS) return refuse(who, "cameras must be in [2, 16]");
    if (rows < 1 || rows > KASF_MATCH_MAX_ROWS) return refuse(who, "rows must be in [1, 64]");
    return frames < 0 || frames > INT32_MAX ? refuse(who, "frames must be in [0, 2^31 - 1]") : 0;
}

}  // namespace

extern "C" {

int64_t kasf_match_workspace_bytes(int32_t cameras, int32_t rows, int64_t frames) {
    if (int rc = refuse_match_shape("match_workspace_bytes", cameras, rows, frames)) return -(int64_t)rc;
    return kasf_match_workspace(cameras, rows, frames);
}

int kasf_match_pair_costs(const float* keypoints, int32_t cameras, int32_t rows, int64_t frames, int32_t joints, const float* camera_rows,
                          const kasf_match_params* params, float* cost, int32_t* samples, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "match_pair_costs";
    if (int rc = refuse_match_shape(who, cameras, rows, frames)) return rc;
    if (joints < 1) return refuse(who, "joints must be >= 1");
    if (frames * joints > INT32_MAX) return refuse(who, "frames * joints must stay below 2^31");
    if (params == nullptr) return refuse_null();
    if (!std::isfinite(params->min_score)) return refuse(who, "min_score must be finite");
    if (params->weighted != 0 && params->weighted != 1) return refuse(who, "weighted must be 0 or 1");
    if (!std::isfinite(params->cap) || !(params->cap > 0.0f)) return refuse(who, "cap must be finite and > 0");
    if (params->min_samples < 1) return refuse(who, "min_samples must be >= 1");
    if (params->undistort_iterations < 0 || params->undistort_iterations > kCamMaxRounds) return refuse(who, "undistort_iterations must be in [0, 20]");
    if (frames == 0) return 0;
    if (!keypoints || !camera_rows || !cost || !samples || !workspace) return refuse_null();
    if (workspace_bytes < kasf_match_workspace(cameras, rows, frames)) return refuse(who, "workspace_bytes is less than kasf_match_workspace_bytes asks for");
    if (((uintptr_t)workspace & 7) != 0) return refuse(who, "workspace must be 8-byte aligned");
    const KasfMatch p{params->min_score, params->cap, params->weighted, params->min_samples, params->undistort_iterations};
    kasf_launch_match_pair_costs((hipStream_t)stream, keypoints, cameras, rows, frames, joints, camera_rows, p, cost, samples, workspace);
    return api_done();
}

int kasf_match_groups(const float* cost, const int32_t* samples, int32_t cameras, int32_t rows, float max_cost, int32_t max_groups, int32_t* group,
                      int32_t* members, int32_t* views, float* group_cost, int32_t* count, int32_t* dropped, void* stream) {
    const char* who = "match_groups";
    if (int rc = refuse_match_shape(who, cameras, rows, 0)) return rc;
    if (!std::isfinite(max_cost) || !(max_cost > 0.0f)) return refuse(who, "max_cost must be finite and > 0");
    if (max_groups < 1 || max_groups > KASF_MATCH_MAX_ROWS) return refuse(who, "max_groups must be in [1, 64]");
    if (!cost || !samples || !group || !members || !views || !group_cost || !count || !dropped) return refuse_null();
    kasf_launch_match_groups((hipStream_t)stream, cost, samples, cameras, rows, max_cost, max_groups, group, members, views, group_cost, count, dropped);
    return api_done();
}

}  // extern "C"
