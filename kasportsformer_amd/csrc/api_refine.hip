// The C entry point of the recorded-track refinement (kasf.h, kasf_tracks_refine), beside api_video.hip's One-Euro entries: it checks its arguments before a
// device or a device pointer is touched, with api_check.h's refusals, and launches k_refine.hip's kernel.
#include "api_check.h"

extern "C" {

int kasf_tracks_refine(const float* x, const int64_t* offsets, int64_t N, int32_t P, int32_t J, int32_t C, int32_t has_score, const kasf_refine_params* params,
                       float* out, uint8_t* state, void* stream) {
    const char* who = "tracks_refine";
    if (J < 1 || J > 256) return refuse(who, "J must be in [1, 256]");
    if (C < 1 || C > 4) return refuse(who, "C must be in [1, 4]");
    if (P < 0 || N < 0) return refuse(who, "P and N must be >= 0");
    if (params == nullptr) return refuse_null();
    if (params->max_gap < 0 || params->max_gap > kRefineMaxGap) return refuse(who, "max_gap must be in [0, 64]");
    if (params->radius < 0 || params->radius > kRefineMaxRadius) return refuse(who, "radius must be in [0, 32]");
    if (!std::isfinite(params->min_score)) return refuse(who, "min_score must be finite");
    KasfRefine p{params->min_score, params->max_gap, params->radius, {}};
    for (int k = 0; k <= kRefineMaxRadius; ++k) {
        const float w = k <= params->radius ? params->weights[k] : 0.0f;       // entries above radius are ignored: the kernel gets zeros
        if (!(w >= 0.0f && w <= 1e6f)) return refuse(who, "weights[0 .. radius] must be finite, not negative and at most 1e6");
        p.w[k] = w;
    }
    if (!(p.w[0] > 0.0f)) return refuse(who, "weights[0] must be > 0");
    if (P == 0 || N == 0) return 0;
    if (!x || !offsets || !out) return refuse_null();
    kasf_launch_tracks_refine((hipStream_t)stream, x, offsets, N, P, J, C, has_score ? 1 : 0, p, out, state);
    return api_done();
}

}  // extern "C"
