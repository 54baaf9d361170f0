// csrc/k_match.hip compiled for the host (tests/test_match_host_cpu.py).  Each entry returns whether a block wrote past the LDS its launch asked for: the pair
// kernel asks for its planes, camera rows and flags; the finish and the grouping kernels' LDS is static, so they ask for none and any write to the dynamic area
// is an overrun.
#include "kernels.h"
#include "k_match.hip"
extern "C" int64_t emul_match_workspace(int C, int P, int64_t N) { return kasf_match_workspace(C, P, N); }
extern "C" int emul_match_pair_costs(const float* keypoints, int C, int P, int64_t N, int J, const float* cameras, float min_score, int weighted, float cap,
                                     int min_samples, int undistort_iterations, float* cost, int* samples, void* workspace) {
    const KasfMatch p{min_score, cap, weighted, min_samples, undistort_iterations};
    g_lds_overrun = 0;
    kasf_launch_match_pair_costs(nullptr, keypoints, C, P, N, J, cameras, p, cost, samples, workspace);
    return g_lds_overrun;
}
extern "C" int emul_match_groups(const float* cost, const int* samples, int C, int P, float max_cost, int G, int* group, int* members, int* views,
                                 float* group_cost, int* count, int* dropped) {
    g_lds_overrun = 0;
    kasf_launch_match_groups(nullptr, cost, samples, C, P, max_cost, G, group, members, views, group_cost, count, dropped);
    return g_lds_overrun;
}
