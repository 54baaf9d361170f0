// The prologue's backward with respect to the input keypoints (gfx950): dx [frames][17][3] fp32 from the three input gradients the embedding backward
// leaves (din3 of kasf_launch_embed_bwd): a = d/d(joints_embed input), b = d/d(bone3), c = d/d(limb3), each [frames][17][3] fp32, a null one = zero.
//   dx = a                                                                         (joints_embed reads x itself, all three channels)
//      + bone_decomposer^T b      (KASportsFormer.py:42-62; k_prologue_fwd's bone lanes)  channels x, y only
//      + sum over the 51 limb-refusion MLPs of their input gradients times c        (bone_refusion.py / bone_MLP.py; k_prologue_fwd's limb lanes, on the RAW joints)
// This file takes KASF_J and gelu_and_grad from common.h and nothing else, so that tests/host_emul/emul_input_grad.cpp can compile it whole for the host.
//
// One wavefront owns one frame: a workgroup of four walks frames IG_FPB at a time with a grid stride.  Lane t < 51 is limb MLP t = (group, channel) with its
// 96 parameters in registers (staged once per workgroup through LDS, zero-padded to four inputs); lanes < 16 then take a bone each.  Both leave their
// contributions in LDS, and after one barrier lane e < 51 GATHERS element e = (joint, channel) of dx through the constant inverse tables below, adding in
// ONE FIXED ORDER:   dx[j][ch] = ((a[j][ch] + bones of joint j by ascending bone index (+gv as the child, -gv as the parent))
//                                             + limb-MLP inputs that read joint j by ascending (group, slot)),   each + one fp32 addition, left to right.
// No atomics: the bits of a frame's dx depend on that frame's operands only -- not on the run, the grid or the other frames of the call.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int IG_FPB = 4;              // frames per workgroup step = wavefronts per workgroup
constexpr int IG_GRID_CAP = 512;       // workgroups: a workgroup's second walk starts at frame IG_FPB * IG_GRID_CAP = 2,048
constexpr int IG_PAR = 96;             // staged floats per MLP: fc1.weight [16][4] (inputs past n: 0) | fc1.bias [16] | fc2.weight [16]
constexpr int IG_PITCH = IG_PAR + 1;
constexpr int IG_BONE_SLOTS = 4, IG_LIMB_SLOTS = 6;

// KASportsFormer.py:46-47 and bone_refusion.py:34-40 (the tables of k_misc.hip, copied as data) and their inverses: for joint j, bone_inv[j] lists
// +(k + 1) / -(k + 1) for every bone k with child / parent j, limb_inv[j] lists 4 * group + slot for every limb-MLP input that reads joint j; both ascending,
// 0 / -1 ends a list
struct IgTables {
    int child[16], parent[16], limb_n[17], limb_idx[17][4];
    int bone_inv[KASF_J][IG_BONE_SLOTS], limb_inv[KASF_J][IG_LIMB_SLOTS];
    bool fits;
};
constexpr IgTables ig_make_tables() {
    IgTables t{{0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15},
               {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16},
               {3, 3, 2, 2, 3, 3, 4, 4, 4, 4, 3, 4, 4, 4, 4, 2, 2},
               {{0, 1, 2, 0}, {3, 4, 5, 0}, {6, 7, 0, 0}, {8, 9, 0, 0}, {10, 11, 12, 0}, {13, 14, 15, 0}, {6, 7, 1, 2}, {6, 7, 4, 5}, {6, 7, 11, 12},
                {6, 7, 14, 15}, {6, 7, 9, 0}, {14, 15, 11, 12}, {1, 2, 4, 5}, {14, 15, 4, 5}, {11, 12, 4, 5}, {10, 0, 0, 0}, {13, 3, 0, 0}},
               {}, {}, true};
    for (int j = 0; j < KASF_J; ++j) {
        int nb = 0, nl = 0;
        for (int s = 0; s < IG_BONE_SLOTS; ++s) t.bone_inv[j][s] = 0;
        for (int s = 0; s < IG_LIMB_SLOTS; ++s) t.limb_inv[j][s] = -1;
        for (int k = 0; k < 16; ++k) {
            if (t.child[k] == j) { if (nb < IG_BONE_SLOTS) t.bone_inv[j][nb] = k + 1; ++nb; }
            if (t.parent[k] == j) { if (nb < IG_BONE_SLOTS) t.bone_inv[j][nb] = -(k + 1); ++nb; }
        }
        for (int i = 0; i < 17; ++i)
            for (int k = 0; k < t.limb_n[i]; ++k)
                if (t.limb_idx[i][k] == j) { if (nl < IG_LIMB_SLOTS) t.limb_inv[j][nl] = i * 4 + k; ++nl; }
        if (nb > IG_BONE_SLOTS || nl > IG_LIMB_SLOTS) t.fits = false;
    }
    return t;
}
static_assert(ig_make_tables().fits, "a joint occurs in more bones / limb-MLP inputs than the inverse tables hold");
__constant__ IgTables c_ig = ig_make_tables();

__global__ __launch_bounds__(64 * IG_FPB) void k_input_grad(const float* __restrict__ x, const float* __restrict__ P, const KasfProOff* __restrict__ offp,
                                                            const float* __restrict__ ga, const float* __restrict__ gb, const float* __restrict__ gc,
                                                            float* __restrict__ dx, int64_t frames) {
    __shared__ float sPar[51 * IG_PITCH];               // staging only: [MLP][IG_PAR] behind an odd pitch (lane t reads row t: no two lanes on one bank)
    __shared__ float sLimb[IG_FPB][3][17 * 4];          // [frame slot][channel][group * 4 + input slot]: the limb MLPs' input gradients
    __shared__ float sBone[IG_FPB][16][2];              // [frame slot][bone][x, y]: gv
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool mlp_lane = lane < 51 && gc != nullptr;
    const int gi = lane < 51 ? lane / 3 : 0, ch = lane < 51 ? lane % 3 : 0;      // as MLP lane: (group, channel); as gather lane: (joint, channel)

    // ---- the 51 MLPs' parameters: global -> LDS (every thread of the workgroup), LDS -> this lane's registers ----
    float w1[16][4], b1[16], w2[16];
    if (gc != nullptr) {                                 // block-uniform
        for (int idx = threadIdx.x; idx < 51 * IG_PAR; idx += 64 * IG_FPB) {
            const int t = idx / IG_PAR, r = idx % IG_PAR, n = c_ig.limb_n[t / 3];
            const int64_t* o = offp->mlp[t];
            float v;
            if (r < 64) v = (r & 3) < n ? P[o[0] + (r >> 2) * n + (r & 3)] : 0.f;
            else if (r < 80) v = P[o[1] + (r - 64)];
            else v = P[o[2] + (r - 80)];
            sPar[t * IG_PITCH + r] = v;
        }
        __syncthreads();
        const float* mine = sPar + (lane < 51 ? lane : 0) * IG_PITCH;
#pragma unroll
        for (int h = 0; h < 16; ++h) {
#pragma unroll
            for (int k = 0; k < 4; ++k) w1[h][k] = mine[h * 4 + k];
            b1[h] = mine[64 + h];
            w2[h] = mine[80 + h];
        }
    }

    for (int64_t f0 = (int64_t)blockIdx.x * IG_FPB; f0 < frames; f0 += (int64_t)gridDim.x * IG_FPB) {      // block-uniform trip count
        const int64_t f = f0 + wave;
        const bool live = f < frames;
        const float* xf = x + f * 51;
        __syncthreads();                                 // the previous step's gather has read sLimb / sBone
        if (live && mlp_lane) {                          // limb MLP (gi, ch): din_k = d sum_h w2_h gelu'(z_h) w1_hk
            float in[4], din[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) in[k] = k < c_ig.limb_n[gi] ? xf[c_ig.limb_idx[gi][k] * 3 + ch] : 0.f;
            const float d = gc[f * 51 + lane];
#pragma unroll
            for (int h = 0; h < 16; ++h) {
                const float z = b1[h] + w1[h][0] * in[0] + w1[h][1] * in[1] + w1[h][2] * in[2] + w1[h][3] * in[3];
                float gz, dgz;
                gelu_and_grad(z, gz, dgz);
                const float dz = d * w2[h] * dgz;
#pragma unroll
                for (int k = 0; k < 4; ++k) din[k] += dz * w1[h][k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) sLimb[wave][ch][gi * 4 + k] = din[k];
        }
        if (live && lane < 16 && gb != nullptr) {        // bone `lane`: b' = b + b_16 / 16 (row 16 of bone3 is the mean of rows 0..15), v = child - parent on (x, y)
            const int c = c_ig.child[lane], p = c_ig.parent[lane];
            const float* bf = gb + f * 51;
            const float b0 = bf[lane * 3] + bf[48] * (1.0f / 16.0f), bb1 = bf[lane * 3 + 1] + bf[49] * (1.0f / 16.0f), b2 = bf[lane * 3 + 2] + bf[50] * (1.0f / 16.0f);
            const float vx = xf[c * 3] - xf[p * 3], vy = xf[c * 3 + 1] - xf[p * 3 + 1];
            const float len = sqrtf(vx * vx + vy * vy);
            float g0 = b0, g1 = bb1;                     // len == 0: the forward used the constant 1 for the length
            if (len != 0.f) {
                const float ux = vx / len, uy = vy / len, dot = ux * b0 + uy * bb1;
                g0 = (b0 - ux * dot) / len + b2 * ux;
                g1 = (bb1 - uy * dot) / len + b2 * uy;
            }
            sBone[wave][lane][0] = g0;
            sBone[wave][lane][1] = g1;
        }
        __syncthreads();
        if (live && lane < 51) {                         // gather element (joint gi, channel ch) in the fixed order of the header
            float acc = ga != nullptr ? ga[f * 51 + lane] : 0.f;
            if (gb != nullptr && ch < 2) {
#pragma unroll
                for (int s = 0; s < IG_BONE_SLOTS; ++s) {
                    const int code = c_ig.bone_inv[gi][s];
                    if (code > 0) acc += sBone[wave][code - 1][ch];
                    else if (code < 0) acc -= sBone[wave][-code - 1][ch];
                }
            }
            if (gc != nullptr) {
#pragma unroll
                for (int s = 0; s < IG_LIMB_SLOTS; ++s) {
                    const int code = c_ig.limb_inv[gi][s];
                    if (code >= 0) acc += sLimb[wave][ch][code];
                }
            }
            dx[f * 51 + lane] = acc;
        }
    }
}

}  // namespace

void kasf_launch_input_grad(hipStream_t s, const float* x, const float* params, const KasfProOff* off, const float* dx_joint3, const float* dbone3,
                            const float* dlimb3, float* dx, int64_t frames) {
    const int64_t steps = (frames + IG_FPB - 1) / IG_FPB;
    const unsigned grid = (unsigned)(steps > IG_GRID_CAP ? IG_GRID_CAP : (steps < 1 ? 1 : steps));
    hipLaunchKernelGGL(k_input_grad, dim3(grid), dim3(64 * IG_FPB), 0, s, x, params, off, dx_joint3, dbone3, dlimb3, dx, frames);
}
