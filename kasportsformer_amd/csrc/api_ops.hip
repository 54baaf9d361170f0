// The C entry points around the model (kasf.h): loss, optimizer, data and evaluation, then the kasf_op_* entries that run one kernel family on its own for the
// unit tests.  The entries that read a kasf_model are in engine.hip.  Every refusal returns before any device call.
#include <cstring>
#include <initializer_list>

#include "api_check.h"

extern "C" {

int kasf_loss3(const float* pred, const float* target, float* dpred, float* losses, int64_t losses_floats, int32_t batch, int32_t n_frames,
               float lambda_n_mpjpe, float lambda_velocity, float grad_scale, void* stream) {
    if (!pred || !target || !dpred || !losses) return refuse_null();
    if (batch < 1 || n_frames < 1) return kasf_set_error(2, "loss3: batch and n_frames must be positive");
    if (losses_floats < 4 + 4 * (int64_t)batch) return kasf_set_error(5, "loss3: `losses` must hold 4 + 4 * batch floats (the per-clip sums live behind the result)");
    kasf_launch_loss3((hipStream_t)stream, pred, target, dpred, losses, batch, n_frames, lambda_n_mpjpe, lambda_velocity, grad_scale);
    return api_done();
}

int kasf_loss7(const float* pred, const float* target, float* dpred, float* losses, int64_t losses_floats, int32_t batch, int32_t n_frames,
               const float* lambdas, float grad_scale, void* stream) {
    if (!pred || !target || !dpred || !losses || !lambdas) return refuse_null();
    if (batch < 1 || n_frames < 1) return kasf_set_error(2, "loss7: batch and n_frames must be positive");
    if (n_frames > KASF_LOSS7_MAX_FRAMES) return kasf_set_error(2, "loss7: n_frames above KASF_LOSS7_MAX_FRAMES (a clip's angles are held in 64 KB of LDS)");
    if (losses_floats < 8 + 8 * (int64_t)batch) return kasf_set_error(5, "loss7: `losses` must hold 8 + 8 * batch floats (the per-clip sums live behind the result)");
    static_assert(KASF_LOSS7_MAX_FRAMES * 174 + 2048 <= 65536, "k_loss7's LDS at the largest clip");
    kasf_launch_loss7((hipStream_t)stream, pred, target, dpred, losses, batch, n_frames, lambdas, grad_scale);
    return api_done();
}

int kasf_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int32_t step_index, float grad_scale, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq) return refuse_null();
    if (n % 4 != 0 || step_index < 1) return kasf_set_error(2, "n must be a multiple of 4 and step_index >= 1");
    // torch.optim.AdamW forms the bias corrections in double (1 - 0.999^t cancels badly in fp32 at small t)
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step_index)), bc2 = (float)(1.0 - pow((double)beta2, (double)step_index));
    kasf_launch_adamw((hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale);
    return api_done();
}

int kasf_adamw_segments(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const KasfOptChunk* chunks, int64_t n_chunks,
                        const KasfAdamwClass* classes, int32_t n_classes, float grad_scale, const float* clip, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !classes || (!chunks && n_chunks != 0)) return refuse_null();
    if (misaligned16(params) || misaligned16(grads) || misaligned16(exp_avg) || misaligned16(exp_avg_sq))
        return kasf_set_error(2, "adamw_segments: the four arrays must be 16-byte aligned");
    if (n < 0 || n_chunks < 0) return kasf_set_error(2, "adamw_segments: negative count");
    if (n_classes < 1 || n_classes > KASF_OPT_MAX_CLASSES) return kasf_set_error(2, "adamw_segments: n_classes outside 1..KASF_OPT_MAX_CLASSES (split the table)");
    KasfAdamwClasses by_value;
    memset(&by_value, 0, sizeof(by_value));
    for (int k = 0; k < n_classes; ++k) {
        KasfAdamwClass& c = by_value.c[k];
        c = classes[k];
        if (c.step < 1) return kasf_set_error(2, "adamw_segments: a class's step must be >= 1");
        // torch.optim.AdamW forms the bias corrections in double, as kasf_adamw_step above
        c.bc1 = (float)(1.0 - pow((double)c.beta1, (double)c.step));
        c.bc2 = (float)(1.0 - pow((double)c.beta2, (double)c.step));
    }
    if (n_chunks == 0) return 0;
    kasf_launch_adamw_segments((hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, chunks, n_chunks, by_value, grad_scale, clip, KASF_OPT_GRID_CAP);
    return api_done();
}

int kasf_grad_norm(const float* grads, int64_t n, const KasfOptChunk* chunks, int64_t n_chunks, double* partial, float grad_scale, float max_norm, float* out2,
                   void* stream) {
    if (!grads || !out2 || ((!chunks || !partial) && n_chunks != 0)) return refuse_null();
    if (misaligned16(grads)) return kasf_set_error(2, "grad_norm: grads must be 16-byte aligned");
    if (n < 0 || n_chunks < 0) return kasf_set_error(2, "grad_norm: negative count");
    if (n_chunks == 0) return 0;
    kasf_launch_grad_norm((hipStream_t)stream, grads, chunks, n_chunks, partial, grad_scale, max_norm, out2, KASF_OPT_GRID_CAP);
    return api_done();
}

int kasf_gather_clips(const float* x_all, const float* y_all, const int64_t* index, const uint8_t* flip, int64_t n_clips, int32_t batch,
                      int32_t n_frames, float* x_out, float* y_out, void* stream) {
    if (!x_all || !index || !x_out || (y_all && !y_out)) return refuse_null();
    if (n_clips < 1 || n_frames < 1) return kasf_set_error(2, "gather_clips: empty clip set");
    kasf_launch_gather_clips((hipStream_t)stream, x_all, y_all, index, flip, n_clips, batch, n_frames, x_out, y_out);
    return api_done();
}
int kasf_joint_flip(const float* src, float* dst, int64_t rows, void* stream) {
    if (!src || !dst || src == dst) return kasf_set_error(2, "joint_flip: null or aliased pointers");
    kasf_launch_joint_flip((hipStream_t)stream, src, dst, rows);
    return api_done();
}
int kasf_tta_merge(const float* pred, const float* pred_of_flipped, float* out, int64_t rows, void* stream) {
    if (!pred || !out) return refuse_null();
    kasf_launch_tta_merge((hipStream_t)stream, pred, pred_of_flipped, out, rows);
    return api_done();
}
int kasf_eval_metrics(const float* pred, const float* label_scaled, const float* factor, const float* res, const int32_t* action, int32_t batch,
                      int32_t n_frames, int32_t n_actions, float* mpjpe, float* p_mpjpe, float* accel, float* jpe, double* action_sums, void* stream) {
    if (!pred || !label_scaled || !factor || !res || !mpjpe || !p_mpjpe || !accel || !jpe) return refuse_null();
    if (n_frames < 3 || n_frames > 256) return kasf_set_error(2, "eval_metrics: n_frames must be in [3,256]");
    if ((action == nullptr) != (action_sums == nullptr)) return kasf_set_error(2, "eval_metrics: action and action_sums go together");
    api_clear_error();
    kasf_launch_eval_metrics((hipStream_t)stream, pred, label_scaled, factor, res, action, batch, n_frames, n_actions, mpjpe, p_mpjpe, accel, jpe, action_sums);
    return api_done(api_launchers_spoke());
}

#define OP_DT_CHECK(dt) \
    if ((dt) != KASF_F32 && (dt) != KASF_BF16) return kasf_set_error(3, "bad dtype")

int kasf_op_linear(int32_t dtype, const void* a, const void* w, const float* bias, void* y, int64_t M, int32_t N, const float* ln_g, const float* ln_b,
                   void* xn_out, int32_t act, void* stream) {
    OP_DT_CHECK(dtype);
    if (N % 128 != 0) return kasf_set_error(2, "N must be a multiple of 128");
    kasf_launch_linear(dtype, (hipStream_t)stream, a, 128, w, 128, bias, y, N, M, N, ln_g, ln_b, xn_out, act);
    return api_done();
}
int kasf_op_linear_res(int32_t dtype, const void* a, const void* w, const float* bias, const float* ls, const void* resid, void* out, int64_t M, void* stream) {
    OP_DT_CHECK(dtype);
    if (!a || !w || !bias || !ls || !resid || !out) return refuse_null();
    kasf_launch_linear_res(dtype, (hipStream_t)stream, a, w, bias, ls, resid, out, M);
    return api_done();
}
int kasf_op_mlp_fwd(int32_t dtype, const void* x, const float* ln_g, const float* ln_b, const void* w1, const float* b1, const void* w2, const float* b2,
                    const float* ls2, void* out, int64_t M, void* xn_out, void* stream) {
    OP_DT_CHECK(dtype);
    kasf_launch_mlp_fwd(dtype, (hipStream_t)stream, x, ln_g, ln_b, w1, b1, w2, b2, ls2, out, M, xn_out);
    return api_done();
}
int kasf_op_mlp_bwd(int32_t dtype, const void* x, const void* g, const float* ln_g, const float* ln_b, const void* w1, const float* b1,
                    const void* w2t_scaled, const void* w1t, void* hbuf, void* dzbuf, void* g_in, float* dgamma, float* dbeta, int64_t M, void* stream) {
    return kasf_op_mlp_bwd_rows(dtype, x, g, ln_g, ln_b, w1, b1, w2t_scaled, w1t, hbuf, dzbuf, g_in, dgamma, dbeta, M, nullptr, 0, stream);
}
int kasf_op_mlp_bwd_fused(const void* x, const void* xn, const void* g, const float* ln_g, const void* w1, const float* b1, const void* w2t_scaled,
                          const void* w1t, void* dapart, float* partial, float* dw1, float* dw2_unscaled, float* db1, float* gsum, void* g_in,
                          float* dgamma, float* dbeta, int64_t M, void* stream) {
    if (!x || !xn || !g || !dapart || !partial || !dw1 || !dw2_unscaled || !db1 || !gsum || !g_in) return refuse_null();
    kasf_launch_mlp_bwd_q((hipStream_t)stream, x, xn, g, ln_g, w1, b1, w2t_scaled, w1t, dapart, partial, dw1, dw2_unscaled, db1, gsum, g_in, dgamma,
                          dbeta, M);
    return api_done();
}
// ---- the same launches with a column sink of their own, finished on the same stream: the form a backward stage runs (kasf.h, kasf_op_sink_scratch_floats ...) ----
// what KasfColSink::take hands out for one request
static int64_t sink_take_floats(int64_t rows, int64_t ld) { return (rows * ld + 63) / 64 * 64; }
int64_t kasf_op_sink_scratch_floats(int32_t op, int32_t dtype, int64_t M, int32_t Kd, int32_t form) {
    if (M < 1) { kasf_set_error(2, "sink_scratch_floats: M must be >= 1"); return -2; }
    if (op < KASF_SINK_MLP_BWD_FUSED_FC2 || op > KASF_SINK_GCN_BWD_ROWS) { kasf_set_error(2, "sink_scratch_floats: unknown op"); return -2; }
    if (op != KASF_SINK_MLP_BWD_FUSED_FC2 && dtype != KASF_F32 && dtype != KASF_BF16) { kasf_set_error(2, "sink_scratch_floats: bad dtype"); return -2; }
    if (op == KASF_SINK_MLP_BWD_FUSED_FC2) {
        int range_rows = 0;
        const int rows = kasf_mlp_bwd_q_rows(M, &range_rows);
        return sink_take_floats(range_rows, 512) + sink_take_floats(rows, 384);
    }
    if (op == KASF_SINK_MLP_BWD_ROWS) return sink_take_floats(kasf_mlp_bwd_rows(dtype, M), 256);
    if (op == KASF_SINK_GCN_BWD_ROWS) return sink_take_floats(kasf_gcn_bwd1_rows(M), 128);
    if (Kd < 128 || Kd % 128 != 0) { kasf_set_error(2, "sink_scratch_floats: Kd must be a positive multiple of 128"); return -2; }
    return sink_take_floats(kasf_dgrad_lnbwd_rows(dtype, Kd, (form & KASF_SINK_FORM_RESID) != 0, (form & KASF_SINK_FORM_DXN_ADD) != 0,
                                                  (form & KASF_SINK_FORM_ACCUMULATE) != 0, (form & KASF_SINK_FORM_XN_OUT) != 0, M), 256);
}
int kasf_op_mlp_bwd_rows(int32_t dtype, const void* x, const void* g, const float* ln_g, const float* ln_b, const void* w1, const float* b1,
                         const void* w2t_scaled, const void* w1t, void* hbuf, void* dzbuf, void* g_in, float* dgamma, float* dbeta, int64_t M, float* scratch,
                         int64_t scratch_floats, void* stream) {
    OP_DT_CHECK(dtype);
    if (int rc = misc_scratch_check(scratch, scratch_floats)) return rc;
    MiscSink ms(scratch, scratch_floats);
    kasf_launch_mlp_bwd(dtype, (hipStream_t)stream, x, g, ln_g, ln_b, w1, b1, w2t_scaled, w1t, hbuf, dzbuf, nullptr, g_in, dgamma, dbeta, M, ms.p);
    return api_done(ms.finish((hipStream_t)stream));
}
int kasf_op_mlp_bwd_fused_fc2(const void* x, const void* xn, const void* g, const float* ln_g, const void* w1, const float* b1, const void* w2t_scaled,
                              const void* w1t, void* dapart, float* partial, float* dw1, float* dw2, float* db1, float* gsum, void* g_in, float* dgamma,
                              float* dbeta, int64_t M, const float* w2, const float* b2, const float* ls2, float* dls2, float* scratch, int64_t scratch_floats,
                              void* stream) {
    if (!x || !xn || !g || !dapart || !partial || !dw1 || !dw2 || !db1 || !gsum || !g_in || !w2 || !b2 || !ls2 || !dls2 || !scratch) return refuse_null();
    if (int rc = misc_scratch_check(scratch, scratch_floats)) return rc;
    if (M <= 0) return 0;
    // no atomics fallback here: without its rows the launch would leave db2 unscaled and dls2 without its b2 term, so a short scratch is refused, not reported behind
    if (scratch_floats < kasf_op_sink_scratch_floats(KASF_SINK_MLP_BWD_FUSED_FC2, KASF_BF16, M, 0, 0))
        return refuse("mlp_bwd_fused_fc2", "scratch_floats is below kasf_op_sink_scratch_floats(KASF_SINK_MLP_BWD_FUSED_FC2): this form has no atomics fallback");
    MiscSink ms(scratch, scratch_floats);
    kasf_launch_mlp_bwd_q((hipStream_t)stream, x, xn, g, ln_g, w1, b1, w2t_scaled, w1t, dapart, partial, dw1, dw2, db1, gsum, g_in, dgamma, dbeta, M, w2, b2, ls2,
                          dls2, ms.p);
    return api_done(ms.finish((hipStream_t)stream));
}
int kasf_op_wgrad(int32_t dtype, const void* g, int32_t N, const void* x, int32_t K, const float* ln_g, const float* ln_b, float* dw, float* dbias,
                  int64_t M, float* partial, int64_t partial_floats, void* stream) {
    OP_DT_CHECK(dtype);
    if (N % 128 != 0 || K % 128 != 0) return kasf_set_error(2, "N and K must be multiples of 128");
    if (ln_g != nullptr && K != 128) return kasf_set_error(2, "LayerNorm-fused wgrad needs K == 128");
    kasf_launch_wgrad(dtype, (hipStream_t)stream, g, N, N, x, K, K, ln_g, ln_b, dw, K, dbias, M, partial, partial_floats);
    return api_done();
}
int kasf_op_dgrad_lnbwd(int32_t dtype, const void* dy, int32_t Kd, const void* wt, const void* dxn_add, const void* x, const float* gamma,
                        const void* resid, void* out, int32_t accumulate, float* dgamma, float* dbeta, int64_t M, void* xn_out, const float* beta,
                        void* stream) {
    return kasf_op_dgrad_lnbwd_rows(dtype, dy, Kd, wt, dxn_add, x, gamma, resid, out, accumulate, dgamma, dbeta, M, xn_out, beta, nullptr, 0, stream);
}
int kasf_op_dgrad_lnbwd_rows(int32_t dtype, const void* dy, int32_t Kd, const void* wt, const void* dxn_add, const void* x, const float* gamma,
                             const void* resid, void* out, int32_t accumulate, float* dgamma, float* dbeta, int64_t M, void* xn_out, const float* beta,
                             float* scratch, int64_t scratch_floats, void* stream) {
    OP_DT_CHECK(dtype);
    if (Kd % 128 != 0) return kasf_set_error(2, "Kd must be a multiple of 128");
    if (xn_out != nullptr && beta == nullptr) return kasf_set_error(2, "xn_out needs beta");
    if (int rc = misc_scratch_check(scratch, scratch_floats)) return rc;
    MiscSink ms(scratch, scratch_floats);
    kasf_launch_dgrad_lnbwd(dtype, (hipStream_t)stream, dy, Kd, wt, dxn_add, x, gamma, resid, out, accumulate, dgamma, dbeta, M, xn_out, beta, ms.p);
    return api_done(ms.finish((hipStream_t)stream));
}
// the fused data + weight gradient launch with a column sink of its own and the finish launches of a backward stage (engine.hip: kasf_launch_bf16_reduce, or
// kasf_launch_proj_finish for the PROJ form, then the sink's flush on the same stream)
int kasf_op_dgrad_wg(const void* dy, int32_t Kd, const void* wt, const void* dxn_add, const void* x, const float* gamma, const float* beta, const void* resid,
                     void* out, int32_t accumulate, float* dgamma, float* dbeta, float* dw, float* dbias, const void* proj_o, const float* proj_w,
                     const float* proj_b, const float* proj_ls, float* dproj_w, float* dproj_b, float* dproj_ls, int64_t M, void* wpart, int64_t wpart_bytes,
                     void* proj_part, int64_t proj_part_bytes, float* scratch, int64_t scratch_floats, void* stream) {
    if (!dy || !wt || !x || !gamma || !beta || !out || !dgamma || !dbeta || !dw || !wpart || !scratch) return refuse_null();
    const int nproj = (proj_o != nullptr) + (proj_w != nullptr) + (proj_b != nullptr) + (proj_ls != nullptr) + (dproj_w != nullptr) + (dproj_b != nullptr) +
                      (dproj_ls != nullptr) + (proj_part != nullptr);
    if (nproj != 0 && nproj != 8) return refuse("dgrad_wg", "proj_o, proj_w, proj_b, proj_ls, dproj_w, dproj_b, dproj_ls and proj_part go together");
    const bool proj = nproj == 8;
    if (Kd < 128 || Kd > 384 || !kasf_dgrad_wg_supported(Kd, resid != nullptr, accumulate != 0, dxn_add != nullptr, dbias != nullptr, proj, 1, INT64_MAX))
        return refuse("dgrad_wg", "not one of the five fused forms (Kd 384 or 128 with resid; Kd 256 accumulating without resid; Kd 256 with resid, dxn_add and dbias; "
                                  "Kd 128 with resid and proj_o)");
    if (wpart_bytes < (int64_t)256 * Kd * 128 * 2) return refuse("dgrad_wg", "wpart_bytes must be at least 256 * Kd * 128 * 2");
    const int64_t proj_tile_bytes = (int64_t)256 * 128 * 128 * 2;
    if (proj && proj_part_bytes < proj_tile_bytes + 256 * 128 * 4) return refuse("dgrad_wg", "proj_part_bytes must be at least 256 * 128 * 128 * 2 + 256 * 128 * 4");
    if (misaligned16(wpart) || (proj && misaligned16(proj_part))) return refuse("dgrad_wg", "wpart and proj_part must be 16-byte aligned");
    if (int rc = misc_scratch_check(scratch, scratch_floats)) return rc;
    if (M <= 0) return 0;
    const int64_t need = ((int64_t)kasf_dgrad_r_rows(M) * (dbias != nullptr ? 512 : 256) + 63) / 64 * 64;
    if (scratch_floats < need) return refuse("dgrad_wg", "scratch_floats is below one row of dgamma | dbeta (| dbias) per workgroup that owns a tile");
    hipStream_t s = (hipStream_t)stream;
    MiscSink ms(scratch, scratch_floats);
    float* pbrow = proj ? (float*)((char*)proj_part + proj_tile_bytes) : nullptr;
    const int np = kasf_launch_dgrad_wg(s, dy, Kd, wt, x, gamma, beta, resid, out, accumulate, dgamma, dbeta, M, ms.p, wpart, wpart_bytes, dxn_add, dbias, proj_o,
                                        proj_part, pbrow);
    if (np <= 0) return kasf_set_error(3, "dgrad_wg: the launcher declined a form that kasf_dgrad_wg_supported accepts");
    const KasfBf16Reduce red{wpart, dw, np, Kd * 128};
    if (proj) kasf_launch_proj_finish(s, proj_part, pbrow, np, dproj_w, proj_w, proj_b, proj_ls, dproj_b, dproj_ls, 1, &red);
    else kasf_launch_bf16_reduce(s, 1, &red);
    return api_done(ms.finish(s));
}
// the streaming weight-gradient launch of an attention / bone block and its finish (engine.hip, block_backward: kasf_launch_wgrad_jobs and nothing else).  The launcher
// returns false for what it cannot run; every such call is refused here first, with the launcher's own split arithmetic restated for the scratch size.
int kasf_op_wgrad_jobs(int32_t njobs, const void* const* g, const void* const* x, const int32_t* N, float* const* dw, float* const* dbias, int32_t fin_job,
                       const float* fin_w, const float* fin_bias, const float* fin_ls, float* dls, int64_t M, float* partial, int64_t partial_floats, int32_t nred,
                       const void* const* red_part, float* const* red_out, const int32_t* red_nparts, const int32_t* red_elems, const void* ext_part,
                       const float* ext_brow, int32_t ext_nparts, float* ext_dw, float* ext_db, void* stream) {
    const char* who = "wgrad_jobs";
    if (njobs < 1 || njobs > 3) return refuse(who, "njobs must be in 1..3");
    if (nred < 0 || nred > 2) return refuse(who, "nred must be in 0..2");
    if (fin_job < -1 || fin_job >= njobs) return refuse(who, "fin_job must be -1 or the index of a job");
    if (M >= ((int64_t)1 << 31)) return refuse(who, "M must stay below 2^31");
    if (!g || !x || !N || !dw || !dbias || !partial || (nred > 0 && (!red_part || !red_out || !red_nparts || !red_elems))) return refuse_null();
    int tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        if (N[j] != 128 && N[j] != 256 && N[j] != 384 && N[j] != 512) return refuse(who, "N[j] must be 128, 256, 384 or 512");
        tiles += N[j] / 128;
    }
    for (int j = 0; j < njobs; ++j)
        if (!g[j] || !x[j] || !dw[j]) return refuse_null();
    for (int k = 0; k < nred; ++k)
        if (!red_part[k] || !red_out[k]) return refuse_null();
    const char* align = "g[j], x[j], dw[j], dbias[j], the fin vectors, partial, red_part[k], red_out[k] and the ext arrays must be 16-byte aligned";
    for (int j = 0; j < njobs; ++j)
        if (misaligned16(g[j]) || misaligned16(x[j]) || misaligned16(dw[j]) || misaligned16(dbias[j])) return refuse(who, align);
    for (int k = 0; k < nred; ++k)
        if (misaligned16(red_part[k]) || misaligned16(red_out[k])) return refuse(who, align);
    for (const void* p : {(const void*)fin_w, (const void*)fin_bias, (const void*)fin_ls, (const void*)dls, (const void*)partial, ext_part, (const void*)ext_brow,
                          (const void*)ext_dw, (const void*)ext_db})
        if (misaligned16(p)) return refuse(who, align);
    for (int j = 0; j < njobs; ++j)
        if (dbias[j] != nullptr && j != fin_job) return refuse(who, "dbias[j] is given on the fin job only (a bias gradient is finished with the layer-scale algebra)");
    if (fin_job >= 0 && (N[fin_job] != 128 || !fin_w || !fin_bias || !fin_ls || !dls || !dbias[fin_job]))
        return refuse(who, "a fin job has N = 128 and needs fin_w, fin_bias, fin_ls, dls and its dbias");
    if (ext_part != nullptr && (fin_job >= 0 || njobs > 2)) return refuse(who, "ext_part goes with fin_job = -1 and at most two jobs");
    const int next = (ext_part != nullptr) + (ext_brow != nullptr) + (ext_nparts >= 1) + (ext_dw != nullptr) + (ext_db != nullptr);
    if (next != 0 && (next != 5 || !fin_w || !fin_bias || !fin_ls || !dls))
        return refuse(who, "ext_part, ext_brow, ext_nparts >= 1, ext_dw and ext_db go together, with fin_w, fin_bias, fin_ls and dls");
    for (int k = 0; k < nred; ++k) {
        if (red_nparts[k] < 1) return refuse(who, "red_nparts[k] must be >= 1");
        if (red_elems[k] < 128 || red_elems[k] % 128 != 0) return refuse(who, "red_elems[k] must be a positive multiple of 128");
    }
    if (M <= 0) return 0;
    // kasf_launch_wgrad_jobs at full width: fewest token splits that fill the chip, slices of whole 128-row tiles
    int64_t splits = (248 + tiles - 1) / tiles;
    splits = std::min(splits, (M + 127) / 128);
    const int64_t slice = ((M + splits - 1) / splits + 127) / 128 * 128;
    splits = (M + slice - 1) / slice;
    int64_t need = 0;
    for (int j = 0; j < njobs; ++j) need += splits * N[j] * 128 + (dbias[j] != nullptr ? splits * N[j] : 0);
    if (partial_floats < need) return refuse(who, "partial_floats is below splits * N[j] * 128 per job (+ splits * 128 for the fin job)");
    KasfBf16Reduce red[2];
    for (int k = 0; k < nred; ++k) red[k] = KasfBf16Reduce{red_part[k], red_out[k], red_nparts[k], red_elems[k]};
    const int Ns[3] = {N[0], njobs > 1 ? N[1] : 0, njobs > 2 ? N[2] : 0};
    if (!kasf_launch_wgrad_jobs((hipStream_t)stream, njobs, g, x, Ns, dw, dbias, fin_job, fin_w, fin_bias, fin_ls, dls, M, partial, partial_floats, nred, red, ext_part,
                                ext_brow, ext_nparts, ext_dw, ext_db))
        return kasf_set_error(3, "wgrad_jobs: the launcher declined a call that passed every check");
    return api_done();
}
// ---- the attention kernels on their own (kasf.h, kasf_op_attention_fwd ... kasf_op_attn_block_fwd): what the five core entries check alike, after their dtype ----
struct AttnLd { const char* name; int64_t ld; };
static int attn_core_check(const char* who, int32_t mode, int32_t batch, int32_t n_frames, std::initializer_list<AttnLd> lds, std::initializer_list<const void*> ptrs) {
    int64_t widest = 384;
    for (const AttnLd& l : lds) widest = std::max(widest, l.ld);
    if (int rc = refuse_attn_shape(who, mode, batch, n_frames, widest)) return rc;
    for (const AttnLd& l : lds)
        if (int rc = refuse_attn_ld(who, l.name, l.ld)) return rc;
    for (const void* p : ptrs)
        if (p == nullptr) return refuse_null();
    for (const void* p : ptrs)              // every kernel behind these entries moves rows in 16-byte pieces (load8 / store8, bf16x8, f32x4), in both dtypes
        if (misaligned16(p)) return refuse(who, "every pointer must be 16-byte aligned");
    return 0;
}
int kasf_op_attention_fwd(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int32_t batch, int32_t n_frames,
                          int32_t mode, void* stream) {
    return kasf_op_attention_fwd_heads(dtype, q, ldq, k, v, ldkv, o, batch, n_frames, mode, 8, stream);
}
int kasf_op_attention_bwd(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* d_o, void* dq, int64_t lddq,
                          void* dk, void* dv, int64_t lddkv, int32_t batch, int32_t n_frames, int32_t mode, void* stream) {
    return kasf_op_attention_bwd_heads(dtype, q, ldq, k, v, ldkv, d_o, dq, lddq, dk, dv, lddkv, batch, n_frames, mode, 8, stream);
}
int kasf_op_attention_fwd_heads(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int32_t batch, int32_t n_frames,
                                int32_t mode, int32_t num_heads, void* stream) {
    OP_DT_CHECK(dtype);
    if (int rc = attn_core_check("attention_fwd", mode, batch, n_frames, {{"ldq", ldq}, {"ldkv", ldkv}}, {q, k, v, o})) return rc;
    if (batch == 0) return 0;
    api_clear_error();
    kasf_launch_attn_fwd(dtype, (hipStream_t)stream, q, ldq, k, v, ldkv, o, batch, n_frames, mode, num_heads);
    return api_done(api_launchers_spoke());
}
int kasf_op_attention_bwd_heads(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* d_o, void* dq, int64_t lddq,
                                void* dk, void* dv, int64_t lddkv, int32_t batch, int32_t n_frames, int32_t mode, int32_t num_heads, void* stream) {
    OP_DT_CHECK(dtype);
    if (int rc = attn_core_check("attention_bwd", mode, batch, n_frames, {{"ldq", ldq}, {"ldkv", ldkv}, {"lddq", lddq}, {"lddkv", lddkv}}, {q, k, v, d_o, dq, dk, dv}))
        return rc;
    if (batch == 0) return 0;
    api_clear_error();
    kasf_launch_attn_bwd(dtype, (hipStream_t)stream, q, ldq, k, v, ldkv, d_o, dq, lddq, dk, dv, lddkv, batch, n_frames, mode, num_heads);
    return api_done(api_launchers_spoke());
}
// (this entry refused batch = 0 before the others learnt to return 0 for it, and keeps doing so: its first three messages and their order are recorded)
int kasf_op_attention_bwd_fused_do(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* g_mid, const void* wproj_t_scaled, void* dq,
                                   int64_t lddq, void* dk, void* dv, int64_t lddkv, int32_t batch, int32_t n_frames, int32_t mode, int32_t form, const void* o_saved,
                                   const float* lse, void* stream) {
    api_clear_error();
    if (form < 0 || form > 1) return kasf_set_error(2, "form: 0 (persistent) or 1 (one group per workgroup)");
    if (batch < 1 || n_frames < 1 || (int64_t)batch * n_frames * 17 * 384 >= ((int64_t)1 << 31)) return kasf_set_error(2, "batch * n_frames * 17 * 384 must stay below 2^31");
    if (int rc = refuse_attn_mode("attention_bwd_fused_do", mode)) return rc;
    const int L = mode == 0 ? 17 : n_frames;
    const char* group = "fused-d_o attention backward: groups of at most 96 positions (form 1: at most 32); bf16, 8 heads";
    if (L > 96 || (form == 1 && L > 32)) return kasf_set_error(2, group);
    if (int rc = attn_core_check("attention_bwd_fused_do", mode, batch, n_frames, {{"ldq", ldq}, {"ldkv", ldkv}, {"lddq", lddq}, {"lddkv", lddkv}},
                                 {q, k, v, g_mid, wproj_t_scaled, dq, dk, dv}))
        return rc;
    if (misaligned16(o_saved) || misaligned16(lse)) return refuse("attention_bwd_fused_do", "every pointer must be 16-byte aligned");
    if (!kasf_launch_attn_bwd_fused_do((hipStream_t)stream, q, ldq, k, v, ldkv, g_mid, wproj_t_scaled, dq, lddq, dk, dv, lddkv, batch, n_frames, mode, form, o_saved, lse))
        return kasf_set_error(2, group);
    return api_done(api_launchers_spoke());
}
// the fused attention block's forward, launched exactly as block_forward (engine.hip) launches it in bf16 mode with 8 heads
int kasf_op_attn_block_fwd(int32_t bone, const void* x, const void* x_limb, const float* ln_g, const float* ln_b, const float* lnl_g, const float* lnl_b, const void* wq,
                           const void* wkv, const void* wproj, const float* bproj, const float* ls1, void* q_save, void* kv_save, void* o_save, float* lse_save,
                           void* out, int32_t batch, int32_t n_frames, int32_t mode, void* stream) {
    const char* who = "attn_block_fwd";
    if (bone != 0 && bone != 1) return refuse(who, "bone must be 0 (self-attention) or 1 (bone cross-attention)");
    if (int rc = refuse_attn_shape(who, mode, batch, n_frames)) return rc;
    const char* group = "the fused kernels cover groups of at most 96 positions (temporal: n_frames <= 96)";
    if ((mode == 0 ? 17 : n_frames) > 96) return refuse(who, group);
    const int nbone = (x_limb != nullptr) + (lnl_g != nullptr) + (lnl_b != nullptr) + (wkv != nullptr);
    if (nbone != (bone ? 4 : 0)) return refuse(who, "x_limb, lnl_g, lnl_b and wkv are all given with bone = 1 and all NULL with bone = 0");
    if ((q_save != nullptr) != (o_save != nullptr)) return refuse(who, "q_save and o_save go together");
    if ((kv_save != nullptr) != (bone && q_save != nullptr)) return refuse(who, "kv_save is given exactly when bone = 1 and q_save / o_save are given");
    if (lse_save != nullptr && q_save == nullptr) return refuse(who, "lse_save needs q_save and o_save");
    if (!x || !ln_g || !ln_b || !wq || !wproj || !bproj || !ls1 || !out) return refuse_null();
    if (out == x || (bone && out == x_limb)) return refuse(who, "out must not alias x or x_limb (a workgroup prefetches the next group's rows while it stores)");
    for (const void* p : {x, x_limb, wq, wkv, wproj, (const void*)q_save, (const void*)kv_save, (const void*)o_save, (const void*)out})
        if (misaligned16(p)) return refuse(who, "x, x_limb, wq, wkv, wproj, q_save, kv_save, o_save and out must be 16-byte aligned");
    if (batch == 0) return 0;
    api_clear_error();
    if (!kasf_launch_attn_block_fwd((hipStream_t)stream, bone, x, x_limb, ln_g, ln_b, lnl_g, lnl_b, wq, wkv, wproj, bproj, ls1, q_save, kv_save, o_save, out, batch, n_frames,
                                    mode, lse_save))
        return refuse(who, group);             // (the launcher's own `false`: the same bound)
    return api_done(api_launchers_spoke());
}
// the fused attention block's backward with the launches that finish it, exactly as block_backward (engine.hip) sequences them in bf16 mode with 8 heads:
// kasf_launch_attn_block_bwd on a local sink, kasf_launch_wgrad_jobs with the ext operands it left, the sink's flush on the same stream
int kasf_op_attn_block_bwd(int32_t bone, const void* x, const void* x_limb, const void* g_mid, const float* ln_g, const float* ln_b, const float* lnl_g, const float* lnl_b,
                           const void* wq, const void* wkv, const void* wq_t, const void* wproj_t_scaled, const float* proj_w, const float* proj_b, const float* ls1,
                           void* out, void* out_limb, void* dq, void* dkv, void* xn_a, void* xn_b, float* dgamma, float* dbeta, float* dgamma_l, float* dbeta_l,
                           float* dw_mix, float* dw_kv, float* dproj_w, float* dproj_b, float* dls1, float* partial, int64_t partial_floats, void* proj_part,
                           int64_t proj_part_bytes, float* scratch, int64_t scratch_floats, int32_t batch, int32_t n_frames, int32_t mode, void* stream) {
    const char* who = "attn_block_bwd";
    if (bone != 0 && bone != 1) return refuse(who, "bone must be 0 (self-attention) or 1 (bone cross-attention)");
    if (int rc = refuse_attn_shape(who, mode, batch, n_frames)) return rc;
    const int L = mode == 0 ? 17 : n_frames;
    if (L > 32) return refuse(who, "the fused backward covers groups of at most 32 positions (temporal: n_frames <= 32)");
    const int nbone = (x_limb != nullptr) + (lnl_g != nullptr) + (lnl_b != nullptr) + (wkv != nullptr) + (wq_t != nullptr) + (out_limb != nullptr) + (dkv != nullptr) +
                      (xn_b != nullptr) + (dgamma_l != nullptr) + (dbeta_l != nullptr) + (dw_kv != nullptr);
    if (nbone != (bone ? 11 : 0))
        return refuse(who, "x_limb, lnl_g, lnl_b, wkv, wq_t, out_limb, dkv, xn_b, dgamma_l, dbeta_l and dw_kv are all given with bone = 1 and all NULL with bone = 0");
    if (!x || !g_mid || !ln_g || !ln_b || !wq || !wproj_t_scaled || !proj_w || !proj_b || !ls1 || !out || !dq || !xn_a || !dgamma || !dbeta || !dw_mix || !dproj_w ||
        !dproj_b || !dls1 || !partial || !proj_part || !scratch)
        return refuse_null();
    if (out == x || (bone && out == x_limb)) return refuse(who, "out must not alias x or x_limb (a workgroup prefetches the next group's rows while it stores)");
    for (const void* p : {x, x_limb, g_mid, wq, wkv, wq_t, wproj_t_scaled, (const void*)proj_w, (const void*)out, (const void*)out_limb, (const void*)dq, (const void*)dkv,
                          (const void*)xn_a, (const void*)xn_b, (const void*)dw_mix, (const void*)dw_kv, (const void*)dproj_w, (const void*)partial, (const void*)proj_part})
        if (misaligned16(p)) return refuse(who, "every bf16 array, proj_w, dw_mix, dw_kv, dproj_w, partial and proj_part must be 16-byte aligned");
    if (int rc = misc_scratch_check(scratch, scratch_floats)) return rc;
    const int64_t proj_tile_bytes = (int64_t)256 * 128 * 128 * 2;
    if (proj_part_bytes < proj_tile_bytes + 256 * 128 * 4) return refuse(who, "proj_part_bytes must be at least 256 * 128 * 128 * 2 + 256 * 128 * 4");
    // kasf_launch_wgrad_jobs at full width over the block's streaming jobs (self: dq | dk | dv, 3 tiles; bone: dq and dk | dv, 1 + 2 tiles), no fin job
    const int64_t M = (int64_t)batch * n_frames * 17;
    int64_t splits = std::min<int64_t>((248 + 2) / 3, (M + 127) / 128);
    if (splits > 0) {
        const int64_t slice = ((M + splits - 1) / splits + 127) / 128 * 128;
        splits = (M + slice - 1) / slice;
    }
    if (partial_floats < splits * 384 * 128) return refuse(who, "partial_floats is below splits * 384 * 128, the streaming weight gradient's partial tiles");
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    MiscSink ms(scratch, scratch_floats);
    float* pbrow = (float*)((char*)proj_part + proj_tile_bytes);
    api_clear_error();
    const int np = kasf_launch_attn_block_bwd(s, bone, x, x_limb, g_mid, ln_g, ln_b, lnl_g, lnl_b, wq, wkv, wq_t, wproj_t_scaled, out, out_limb, dq, dkv, xn_a, xn_b, dgamma,
                                              dbeta, dgamma_l, dbeta_l, ms.p, proj_part, pbrow, batch, n_frames, mode);
    if (np <= 0) {
        if (ms.sink.overflow) return ms.finish(s);      // scratch below one row of dgamma | dbeta (| the limb pair) per active workgroup: error 6, nothing launched
        return kasf_set_error(3, "attn_block_bwd: the launcher declined a call that passed every check");
    }
    const void* Gs[2] = {dq, dkv};
    const void* Xs[2] = {xn_a, xn_b};
    const int Ns[2] = {bone ? 128 : 384, 256};
    float* dWs[2] = {dw_mix, dw_kv};
    float* dbs[2] = {nullptr, nullptr};
    if (!kasf_launch_wgrad_jobs(s, bone ? 2 : 1, Gs, Xs, Ns, dWs, dbs, -1, proj_w, proj_b, ls1, dls1, M, partial, partial_floats, 0, nullptr, proj_part, pbrow, np, dproj_w,
                                dproj_b)) {
        ms.finish(s);
        return kasf_set_error(3, "attn_block_bwd: the weight-gradient launcher declined a call that passed every check");
    }
    return api_done(ms.finish(s));
}
// ---- the GCN mixer on its own (kasf.h, kasf_op_gcn_fwd / kasf_op_gcn_bwd): the launch sequence and `count` of block_forward / block_backward ----
static_assert(KASF_GCN_STAT_WORDS == KASF_STAT_SLOTS * KASF_STAT_LD * KASF_STAT_WORDS, "kasf.h and kernels.h disagree on the size of a statistics buffer");
static int gcn_shape_check(int32_t batch, int32_t n_frames, int32_t mode) {
    if (mode != 0 && mode != 1) return kasf_set_error(2, "gcn: mode must be 0 (spatial) or 1 (temporal)");
    if (n_frames < 4 || n_frames > KASF_MAX_NODES) return kasf_set_error(2, "gcn: n_frames must be in [4, 256]");
    if (batch < 1 || (int64_t)batch * n_frames * 17 * 16 >= ((int64_t)1 << 31)) return kasf_set_error(2, "gcn: batch >= 1 and batch * n_frames * 17 * 16 must stay below 2^31");
    return 0;
}
int kasf_op_gcn_fwd(int32_t dtype, const void* x_in, const void* xn, const void* uv, const float* bn_w, const float* bn_b, float* run_mean, float* run_var,
                    const float* ls1, void* y, uint32_t* mask, void* stats, float* coef, void* out, int32_t batch, int32_t n_frames, int32_t mode,
                    int32_t neighbour_num, int32_t training, float momentum, void* stream) {
    OP_DT_CHECK(dtype);
    if (gcn_shape_check(batch, n_frames, mode) != 0) return 2;
    if (neighbour_num < 1 || neighbour_num > 4) return kasf_set_error(2, "gcn: neighbour_num must be in [1, 4]");
    if (!x_in || !xn || !uv || !bn_w || !bn_b || !run_mean || !run_var || !ls1 || !y || !stats || !coef || !out || (mode == 1 && !mask))
        return refuse_null();
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(stats, 0, (size_t)KASF_GCN_STAT_WORDS * sizeof(int64_t), s));
    kasf_launch_gcn_agg_fwd(dtype, s, uv, xn, y, mode == 1 ? mask : nullptr, (double*)stats, batch, n_frames, mode, neighbour_num);
    const double count = mode == 0 ? (double)batch * n_frames * 128 : (double)batch * 17 * 128;
    kasf_launch_gcn_apply(dtype, s, x_in, xn, y, (const double*)stats, bn_w, bn_b, run_mean, run_var, coef, ls1, out, batch, n_frames, mode, count,
                          training ? 1 : 0, momentum);
    return api_done();
}
int kasf_op_gcn_bwd(int32_t dtype, const void* g, const void* xn, const void* y, const float* coef, const uint32_t* mask, const float* ls1, void* r, void* duv,
                    float* dls1, float* d_bn_w, float* d_bn_b, void* bstats, int32_t batch, int32_t n_frames, int32_t mode, int32_t training, void* stream) {
    return kasf_op_gcn_bwd_rows(dtype, g, xn, y, coef, mask, ls1, r, duv, dls1, d_bn_w, d_bn_b, bstats, batch, n_frames, mode, training, nullptr, 0, stream);
}
int kasf_op_gcn_bwd_rows(int32_t dtype, const void* g, const void* xn, const void* y, const float* coef, const uint32_t* mask, const float* ls1, void* r, void* duv,
                         float* dls1, float* d_bn_w, float* d_bn_b, void* bstats, int32_t batch, int32_t n_frames, int32_t mode, int32_t training, float* scratch,
                         int64_t scratch_floats, void* stream) {
    OP_DT_CHECK(dtype);
    if (gcn_shape_check(batch, n_frames, mode) != 0) return 2;
    if (!g || !xn || !y || !coef || !ls1 || !r || !duv || !dls1 || !d_bn_w || !d_bn_b || !bstats || (mode == 1 && !mask))
        return refuse_null();
    if (int rc = misc_scratch_check(scratch, scratch_floats)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(bstats, 0, (size_t)KASF_GCN_STAT_WORDS * sizeof(int64_t), s));
    MiscSink ms(scratch, scratch_floats);
    kasf_launch_gcn_bwd1(dtype, s, g, xn, y, coef, ls1, r, dls1, (double*)bstats, batch, n_frames, mode, ms.p);
    const double count = mode == 0 ? (double)batch * n_frames * 128 : (double)batch * 17 * 128;
    kasf_launch_gcn_bwd2(dtype, s, r, y, coef, mode == 1 ? mask : nullptr, duv, batch, n_frames, mode, (const double*)bstats, d_bn_w, d_bn_b, count,
                         training ? 1 : 0);
    return api_done(ms.finish(s));
}
// ---- the gate, head and embedding kernels on their own (kasf.h, kasf_op_embed_bwd ... kasf_op_add): the engine's own launchers; the scratch of api_check.h's MiscSink ----
#define MISC_TOKENS_CHECK(M, what) \
    if ((M) < 1 || (int64_t)(M) * 384 >= ((int64_t)1 << 31)) return kasf_set_error(2, what ": 1 <= tokens and tokens * 384 < 2^31")
int kasf_op_embed_bwd(int32_t dtype, const void* g, const float* in3, const float* w, float* dw, float* db, float* dpos, float* din3, int64_t frames,
                      float* scratch, int64_t scratch_floats, void* stream) {
    OP_DT_CHECK(dtype);
    if (!g || !in3 || !w || !dw || !db || !dpos) return refuse_null();
    if (refuse_misc_frames(frames)) return 2;
    if (misc_scratch_check(scratch, scratch_floats)) return 2;
    MiscSink ms(scratch, scratch_floats);
    kasf_launch_embed_bwd(dtype, (hipStream_t)stream, g, in3, w, dw, db, dpos, din3, frames, ms.p);
    return api_done(ms.finish((hipStream_t)stream));
}
int kasf_op_gate_fwd(int32_t dtype, const void* xa, const void* xg, const void* xb, const float* w, const float* bias, void* out, float* alpha, int64_t M,
                     int32_t adaptive, void* stream) {
    OP_DT_CHECK(dtype);
    if (!xa || !xg || !xb || !w || !bias || !out) return refuse_null();
    MISC_TOKENS_CHECK(M, "gate_fwd");
    kasf_launch_gate_fwd(dtype, (hipStream_t)stream, xa, xg, xb, w, bias, out, alpha, M, adaptive ? 1 : 0);
    return api_done();
}
int kasf_op_gate_bwd(int32_t dtype, const void* g, const void* g1, const void* g2, const void* xa, const void* xg, const void* xb, const float* w,
                     const float* alpha, void* ga, void* gg, void* gb, float* dw, float* db, int64_t M, int32_t adaptive, float* scratch,
                     int64_t scratch_floats, void* stream) {
    OP_DT_CHECK(dtype);
    if (!g || !xa || !xg || !xb || !w || !alpha || !ga || !gg || !gb || (adaptive && (!dw || !db))) return refuse_null();
    if (misaligned16(alpha)) return kasf_set_error(2, "gate_bwd: alpha must be 16-byte aligned");
    MISC_TOKENS_CHECK(M, "gate_bwd");
    if (misc_scratch_check(scratch, scratch_floats)) return 2;
    MiscSink ms(scratch, scratch_floats);
    kasf_launch_gate_bwd(dtype, (hipStream_t)stream, g, g1, g2, xa, xg, xb, w, alpha, ga, gg, gb, dw, db, M, adaptive ? 1 : 0, ms.p);
    return api_done(ms.finish((hipStream_t)stream));
}
int kasf_op_head_fwd(int32_t dtype, const void* rep, const float* w, const float* bias, float* out, int64_t M, void* stream) {
    OP_DT_CHECK(dtype);
    if (!rep || !w || !bias || !out) return refuse_null();
    MISC_TOKENS_CHECK(M, "head_fwd");
    kasf_launch_head_fwd(dtype, (hipStream_t)stream, rep, w, bias, out, M);
    return api_done();
}
int kasf_op_head_bwd(int32_t dtype, const float* dy, const void* rep, const float* w, void* dpre, float* dw, float* db, int64_t M, float* scratch,
                     int64_t scratch_floats, void* stream) {
    OP_DT_CHECK(dtype);
    if (!dy || !rep || !w || !dpre || !dw || !db) return refuse_null();
    MISC_TOKENS_CHECK(M, "head_bwd");
    if (misc_scratch_check(scratch, scratch_floats)) return 2;
    MiscSink ms(scratch, scratch_floats);
    kasf_launch_head_bwd(dtype, (hipStream_t)stream, dy, rep, w, dpre, dw, db, M, ms.p);
    return api_done(ms.finish((hipStream_t)stream));
}
int kasf_op_rep_bwd(int32_t dtype, const float* drep, const void* rep, void* dpre, int64_t M, void* stream) {
    OP_DT_CHECK(dtype);
    if (!drep || !rep || !dpre) return refuse_null();
    MISC_TOKENS_CHECK(M, "rep_bwd");
    kasf_launch_rep_bwd(dtype, (hipStream_t)stream, drep, rep, dpre, M);
    return api_done();
}
int kasf_op_finalize_ls(float* dw, const float* w, const float* bias, const float* ls, float* db, float* dls, int32_t N, int32_t K, void* stream) {
    if (!dw || !w || !bias || !ls || !db || !dls) return refuse_null();
    if (N != 128 || (K != 128 && K != 512)) return kasf_set_error(2, "finalize_ls: (N, K) must be (128, 128) or (128, 512), the two layer-scaled Linear layers of a block");
    kasf_launch_finalize_ls((hipStream_t)stream, dw, w, bias, ls, db, dls, N, K);
    return api_done();
}
int kasf_op_add(int32_t dtype, void* dst, const void* a, const void* b, const void* c, int64_t n, void* stream) {
    OP_DT_CHECK(dtype);
    if (!dst || !a || (!b && c)) return kasf_set_error(2, "null pointer argument (c needs b)");
    if (n < 8 || n % 8 != 0 || n >= ((int64_t)1 << 40)) return kasf_set_error(2, "add: n must be a multiple of 8 in [8, 2^40)");
    if (b == nullptr) kasf_launch_add_inplace(dtype, (hipStream_t)stream, dst, a, n);
    else kasf_launch_add3(dtype, (hipStream_t)stream, dst, a, b, c, n);
    return api_done();
}
int kasf_op_cast(int32_t dtype, const void* src, void* dst, int64_t n, int32_t to_f32, void* stream) {
    OP_DT_CHECK(dtype);
    if (to_f32) kasf_launch_cast_to_f32(dtype, (hipStream_t)stream, src, (float*)dst, n);
    else kasf_launch_cast_from_f32(dtype, (hipStream_t)stream, (const float*)src, dst, n);
    return api_done();
}

}  // extern "C"
