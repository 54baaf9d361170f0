// Where a person's crop sits in the frame: the one derivation that k_heatmap.hip (crop -> frame, per keypoint) and k_crop.hip (crop -> frame, per pixel) share.
//   box_to_center_scale                       demo/lib/hrnet/lib/utils/utilitys.py:102-135
//   get_affine_transform with rot = 0, inv    demo/lib/hrnet/lib/utils/transforms.py:58-101
// The library is built with -ffp-contract=off: every expression below rounds where the reference's numpy expression rounds.
#pragma once
#include <hip/hip_runtime.h>

struct KasfCropGeom {
    float cx, cy, sx, sy;    // center, scale as fp32: given (geom_kind 0) or derived from the box (geom_kind 1)
    double kx, ky;           // frame pixels per crop pixel, x and y (both divide by W / 2, as the reference does)
};

// g = the person's four fp32 values; W = the crop's (or heatmap's) width in pixels.  A crop pixel (x, y) sits at frame position
// (cx + (x - W / 2) kx, cy + (y - H / 2) ky), evaluated in fp64 by the caller.
__device__ inline KasfCropGeom kasf_crop_geom(const float* __restrict__ g, int geom_kind, double aspect, int W) {
    KasfCropGeom r;
    float cx, cy, sx, sy;
    if (geom_kind == 0) {
        cx = g[0]; cy = g[1]; sx = g[2]; sy = g[3];
    } else {
        // box_to_center_scale, in fp64 on the upcast box
        const double x1 = g[0], y1 = g[1], x2 = g[2], y2 = g[3];
        double bw = x2 - x1, bh = y2 - y1;
        cx = (float)(x1 + bw * 0.5);
        cy = (float)(y1 + bh * 0.5);
        if (bw > aspect * bh) bh = bw * 1.0 / aspect;
        else if (bw < aspect * bh) bw = bh * aspect;
        sx = (float)(bw * 1.0 / 200.0);
        sy = (float)(bh * 1.0 / 200.0);
        if (cx != -1.0f) { sx = sx * 1.25f; sy = sy * 1.25f; }
    }
    // three anchor points stored as fp32, the affine through them in closed form in fp64; only scale[0] enters
    const float sw = sx * 200.0f;                                        // scale_tmp[0]
    const float s1y = (float)((double)cy + (double)(sw * -0.5f));        // src[1, 1] = center + src_dir, an fp64 sum stored as fp32
    const float dy = cy - s1y;                                           // get_3rd_point: direct = src[0] - src[1]
    const float s2x = cx + (-dy);                                        // src[2, 0] = src[1, 0] - direct[1]
    const double half_w = (double)W * 0.5;
    r.cx = cx; r.cy = cy; r.sx = sx; r.sy = sy;
    r.kx = ((double)cx - (double)s2x) / half_w;
    r.ky = ((double)cy - (double)s1y) / half_w;
    return r;
}
