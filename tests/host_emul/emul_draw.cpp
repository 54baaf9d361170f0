// csrc/k_draw.hip compiled for the host (tests/test_draw_host_cpu.py).
#include "kernels.h"
#include "k_draw.hip"
// -> the number of launches made (the entry point promises one)
extern "C" int emul_draw_poses(const KasfDrawLaunch* d) {
    g_launches = 0;
    kasf_launch_draw_poses(nullptr, d);
    return g_launches;
}
extern "C" int emul_pose_panel(const float* poses, int64_t n, const float* view, float* out) {
    g_launches = 0;
    kasf_launch_pose_panel(nullptr, poses, n, view, out);
    return g_launches;
}
// the kernel's tile and list: { tile width, tile height, list entries, threads, size of KasfDrawLaunch }
extern "C" void emul_draw_constants(int* out) {
    out[0] = DRAW_TILE_W; out[1] = DRAW_TILE_H; out[2] = DRAW_LIST; out[3] = DRAW_THREADS; out[4] = (int)sizeof(KasfDrawLaunch);
}
