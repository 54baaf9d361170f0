// csrc/k_triangulate.hip compiled for the host (tests/test_triangulate_host_cpu.py).  Each entry returns whether a block wrote past the LDS its launch asked
// for: the triangulation asks for its planes, staging tile and camera rows; the undistortion's tile is static, so it asks for none and any write to the
// dynamic area is an overrun.
#include "kernels.h"
#include "k_triangulate.hip"
extern "C" int emul_triangulate(const float* keypoints, int views, int64_t M, int ppf, const float* cameras, int cameras_per_frame, float min_score,
                                int weighted, int iterations, float delta, int min_views, int undistort_iterations, float* points, float* residual,
                                unsigned char* used, unsigned char* state, float* view_residual) {
    const KasfTriangulate p{min_score, delta, weighted, iterations, min_views, undistort_iterations};
    g_lds_overrun = 0;
    kasf_launch_keypoints_triangulate(nullptr, keypoints, views, M, ppf, cameras, cameras_per_frame, p, points, residual, used, state, view_residual);
    return g_lds_overrun;
}
extern "C" int emul_undistort(const float* keypoints, int64_t M, int ppf, const float* camera, int camera_per_frame, int rounds, float* out) {
    g_lds_overrun = 0;
    kasf_launch_keypoints_undistort(nullptr, keypoints, M, ppf, camera, camera_per_frame, rounds, out);
    return g_lds_overrun;
}
