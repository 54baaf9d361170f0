// The C entry points of the multi-camera triangulation and of the lens undistortion (kasf.h, kasf_keypoints_triangulate / kasf_keypoints_undistort), built like
// api_place.hip: they check their arguments before a device or a device pointer is touched, with api_check.h's refusals, and launch k_triangulate.hip's kernels
// (tests/test_triangulate_refusals_cpu.py holds every message here to a case).
#include "api_check.h"
#include "camera_model.h"

extern "C" {

int kasf_keypoints_triangulate(const float* keypoints, int32_t views, int64_t M, int32_t points_per_frame, const float* cameras, int32_t cameras_per_frame,
                               const kasf_triangulate_params* params, float* points, float* residual, uint8_t* used, uint8_t* state, float* view_residual,
                               void* stream) {
    const char* who = "keypoints_triangulate";
    if (views < 2 || views > 16) return refuse(who, "views must be in [2, 16]");
    if (M < 0) return refuse(who, "M must be >= 0");
    if (points_per_frame < 1) return refuse(who, "points_per_frame must be >= 1");
    if (M % points_per_frame != 0) return refuse(who, "M must be a multiple of points_per_frame");
    if (params == nullptr) return refuse_null();
    if (!std::isfinite(params->min_score)) return refuse(who, "min_score must be finite");
    if (params->weighted != 0 && params->weighted != 1) return refuse(who, "weighted must be 0 or 1");
    if (params->iterations < 0 || params->iterations > 8) return refuse(who, "iterations must be in [0, 8]");
    if (!std::isfinite(params->delta) || !(params->delta > 0.0f)) return refuse(who, "delta must be finite and > 0");
    if (params->min_views < 2 || params->min_views > 16) return refuse(who, "min_views must be in [2, 16]");
    if (params->undistort_iterations < 0 || params->undistort_iterations > kCamMaxRounds) return refuse(who, "undistort_iterations must be in [0, 20]");
    if (M == 0) return 0;
    if (!keypoints || !cameras || !points) return refuse_null();
    if (points == keypoints) return refuse(who, "points must be an array of its own, not keypoints");
    const KasfTriangulate p{params->min_score, params->delta, params->weighted, params->iterations, params->min_views, params->undistort_iterations};
    kasf_launch_keypoints_triangulate((hipStream_t)stream, keypoints, views, M, points_per_frame, cameras, cameras_per_frame ? 1 : 0, p, points, residual, used,
                                      state, view_residual);
    return api_done();
}

int kasf_keypoints_undistort(const float* keypoints, int64_t M, int32_t points_per_frame, const float* camera, int32_t camera_per_frame, int32_t iterations,
                             float* out, void* stream) {
    const char* who = "keypoints_undistort";
    if (M < 0) return refuse(who, "M must be >= 0");
    if (points_per_frame < 1) return refuse(who, "points_per_frame must be >= 1");
    if (M % points_per_frame != 0) return refuse(who, "M must be a multiple of points_per_frame");
    if (iterations < 0 || iterations > kCamMaxRounds) return refuse(who, "iterations must be in [0, 20]");
    if (M == 0) return 0;
    if (!keypoints || !camera || !out) return refuse_null();
    if (out == keypoints) return refuse(who, "out must be an array of its own, not keypoints");
    kasf_launch_keypoints_undistort((hipStream_t)stream, keypoints, M, points_per_frame, camera, camera_per_frame ? 1 : 0, iterations, out);
    return api_done();
}

}  // extern "C"
