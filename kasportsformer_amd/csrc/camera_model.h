// The camera model that the triangulation and the undistortion share (kasf.h, kasf_keypoints_triangulate / kasf_keypoints_undistort): one definition of the
// camera row, of "finite" and of the fixed-point undistortion, so that "undistort, then triangulate with zero coefficients" and "triangulate" walk the same
// arithmetic.  The library is built with -ffp-contract=off and a correctly rounded divide and square root: every line below is the rounded fp64 operation(s)
// kasf.h names, by its parentheses, then left to right.
// Plain C++: HIP device code in the library, g++ behind the stand-in hip/hip_runtime.h of tests/host_emul/ in the CPU tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// a camera row: 21 fp32 values
constexpr int kCamFx = 0, kCamFy = 1, kCamCx = 2, kCamCy = 3;          // pixels
constexpr int kCamK1 = 4, kCamK2 = 5, kCamP1 = 6, kCamP2 = 7, kCamK3 = 8;  // Brown-Conrady, OpenCV's order
constexpr int kCamR = 9, kCamT = 18;                                   // R [9] row-major and t [3]: X_cam = R X_world + t
constexpr int kCamFloats = 21, kCamLensFloats = 9;                     // the whole row | the part the undistortion reads
constexpr int kCamMaxRounds = 20;                                      // undistort_iterations in [0, kCamMaxRounds]

// the first n values of a row are finite (false for a NaN and for an infinity)
__device__ inline bool camera_finite(const float* cam, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && fabsf(cam[i]) <= 3.4028235e38f;
    return ok;
}

// pixel (u, v) -> the undistorted normalised point (x, y): `rounds` rounds of the fixed-point iteration, a fixed count with no convergence test (0: a pinhole)
__device__ inline void camera_undistort(const float* cam, float u, float v, int rounds, double& x, double& y) {
    const double fx = (double)cam[kCamFx], fy = (double)cam[kCamFy], cx = (double)cam[kCamCx], cy = (double)cam[kCamCy];
    const double k1 = (double)cam[kCamK1], k2 = (double)cam[kCamK2], p1 = (double)cam[kCamP1], p2 = (double)cam[kCamP2], k3 = (double)cam[kCamK3];
    const double xd = ((double)u - cx) / fx, yd = ((double)v - cy) / fy;
    x = xd;
    y = yd;
    for (int i = 0; i < rounds; ++i) {
        const double r2 = x * x + y * y;
        const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (xd - dx) / rad;
        y = (yd - dy) / rad;
    }
}
