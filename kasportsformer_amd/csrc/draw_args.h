// The arguments of kasf_launch_draw_poses (k_draw.hip), as the entry points of api_video.hip have checked them (kasf.h, kasf_draw_poses): plain data, shared
// with the host build of the kernel's source (tests/host_emul/emul_draw.cpp).
#pragma once
#include <stdint.h>

struct KasfDrawLaunch {
    const void* frames;                 // uint8 [n_frames][Hf][Wf][3] behind row_stride / frame_stride (bytes)
    int n_frames, Hf, Wf;               // Hf, Wf in 1..32767
    int64_t row_stride, frame_stride;
    const float* keypoints;             // [n_frames][P][J][2 or 3] behind four element strides; unused with P * S == 0
    int P, J, use_score;                // use_score != 0: the third coordinate is compared with min_score
    int64_t kp_frame_stride, kp_person_stride, kp_joint_stride, kp_coord_stride;
    const unsigned char* valid;         // [n_frames][P] behind two byte strides, or null
    int64_t valid_frame_stride, valid_person_stride;
    const int* segments;                // [S][2]
    const unsigned char* colors;        // [S][3]
    int S;
    unsigned char dot_color[3];
    int thickness, dot_radius;
    float min_score;
    const int* fills;                   // [R][7]
    int R;
    void* out_bgr;                      // or null
    int64_t out_row_stride, out_frame_stride;
    void *out_y, *out_uv;               // both or neither
    int64_t y_row_stride, uv_row_stride, y_frame_stride, uv_frame_stride;
    const int* coef;                    // rule 5's { CRY, CGY, CBY, CRU, CGU, CH, CGV, CBV } of the chosen matrix and range
    int full_range, rgb;
};
