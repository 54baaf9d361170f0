// The C entry point of the camera-space placement (kasf.h, kasf_pose_place), built like api_refine.hip: it checks its arguments before a device or a device
// pointer is touched, with api_check.h's refusals, and launches k_place.hip's kernel (tests/test_place_refusals_cpu.py holds every message here to a case).
#include "api_check.h"

extern "C" {

int kasf_pose_place(const float* poses, const float* keypoints, int64_t frames, const float* camera, int32_t camera_per_frame, const float* lengths,
                    int32_t lengths_per_frame, const kasf_place_params* params, float* out, float* root, float* residual, float* scale, uint8_t* state,
                    void* stream) {
    const char* who = "pose_place";
    if (frames < 0) return refuse(who, "frames must be >= 0");
    if (params == nullptr) return refuse_null();
    if (!std::isfinite(params->min_score)) return refuse(who, "min_score must be finite");
    if (params->weighted != 0 && params->weighted != 1) return refuse(who, "weighted must be 0 or 1");
    if (params->iterations < 0 || params->iterations > 8) return refuse(who, "iterations must be in [0, 8]");
    if (!std::isfinite(params->delta) || !(params->delta > 0.0f)) return refuse(who, "delta must be finite and > 0");
    if (params->min_joints < 2 || params->min_joints > 17) return refuse(who, "min_joints must be in [2, 17]");
    if (frames == 0) return 0;
    if (!poses || !keypoints || !camera || !out) return refuse_null();
    if (out == poses || out == keypoints) return refuse(who, "out must be an array of its own, neither poses nor keypoints");
    const KasfPlace p{params->min_score, params->delta, params->weighted, params->iterations, params->min_joints};
    kasf_launch_pose_place((hipStream_t)stream, poses, keypoints, frames, camera, camera_per_frame ? 1 : 0, lengths, lengths_per_frame ? 1 : 0, p, out, root,
                           residual, scale, state);
    return api_done();
}

}  // extern "C"
