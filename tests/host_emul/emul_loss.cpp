// csrc/k_loss.hip compiled for the host (tests/test_loss_host_cpu.py): a copy of the kernel in the build directory, so that its #include "common.h" finds the
// stand-in of this directory.  k_loss3.inc is written by the test: the k_loss3 / k_loss3_finish / kasf_launch_loss3 text of csrc/k_misc.hip cut out as it is,
// with its dynamic-LDS declaration replaced by the stand-in's, for the bit comparison of the three old terms.
#include "kernels.h"
#include "k_loss.hip"
#include "k_loss3.inc"
extern "C" int emul_loss7(const float* pred, const float* tgt, float* dpred, float* losses, int B, int T, const float* lambdas, float grad_scale) {
    g_launches = 0;
    kasf_launch_loss7(nullptr, pred, tgt, dpred, losses, B, T, lambdas, grad_scale);
    return g_launches;
}
extern "C" int emul_loss3(const float* pred, const float* tgt, float* dpred, float* losses, int B, int T, float lambda_n, float lambda_v, float grad_scale) {
    g_launches = 0;
    kasf_launch_loss3(nullptr, pred, tgt, dpred, losses, B, T, lambda_n, lambda_v, grad_scale);
    return g_launches;
}
