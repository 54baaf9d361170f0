// csrc/k_place.hip compiled for the host (tests/test_place_host_cpu.py).  Returns whether a block wrote past the LDS its launch asked for (the kernel's two
// tiles are static, so the launch asks for none and any write to the dynamic area is an overrun).
#include "kernels.h"
#include "k_place.hip"
extern "C" int emul_place(const float* poses, const float* keypoints, int64_t frames, const float* camera, int camera_per_frame, const float* lengths,
                          int lengths_per_frame, float min_score, int weighted, int iterations, float delta, int min_joints, float* out, float* root,
                          float* residual, float* scale, unsigned char* state) {
    const KasfPlace p{min_score, delta, weighted, iterations, min_joints};
    g_lds_overrun = 0;
    kasf_launch_pose_place(nullptr, poses, keypoints, frames, camera, camera_per_frame, lengths, lengths_per_frame, p, out, root, residual, scale, state);
    return g_lds_overrun;
}
