/* libkasf_hip -- C-ABI of the MI355X-native (gfx950) KASportsFormer forward/backward path.
 *
 * The reference (jw0r1n/KASportsFormer) is pure Python/PyTorch: its "FFI" for this path is the
 * nn.Module call  KASportsFormer.forward(x[B,T,17,3]) -> [B,T,17,3]  plus autograd.  This header is
 * the boundary a reference maintainer binds instead (ctypes stub in INTEGRATION.md): plain pointers
 * and sizes, no torch types.  All pointers are DEVICE pointers owned by the caller (torch's caching
 * allocator in the shipped host code); `stream` is a hipStream_t passed as void*.  Nothing here
 * allocates, frees or synchronises in the hot path (graph-capture safe); only kasf_model_create()
 * allocates a few KB of device tables.
 *
 * Every function returns 0 on success or a non-zero code; kasf_last_error() describes it.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   kasf_model_create      <- KASportsFormer.__init__             model/KASportsFormer.py:291-318
 *   kasf_param_*           <- nn.Module.state_dict() layout       model/KASportsFormer.py:296-318 (names identical)
 *   kasf_forward           <- KASportsFormer.forward              model/KASportsFormer.py:320-347
 *   kasf_backward          <- torch.autograd of the above         train_and_evaluate_sp.py:241  (loss.backward()); with KASF_FLAG_INPUT_GRAD also x.grad
 *   kasf_loss3             <- mpjpe + 0.5 n_mpjpe + 20 velocity   utils/loss_calc.py:6-27, train_and_evaluate_sp.py:212-222
 *   kasf_loss7             <- the complete seven-term loss: the three above + lambda_limb_len_var loss_limb_var_calc + lambda_limb_len loss_limb_len_calc
 *                             + lambda_limb_cos_simi loss_cos_simi_calc + lambda_limb_cos_simi_velocity loss_cos_simi_velocity_calc
 *                             utils/loss_calc.py:30-94, train_and_evaluate_sp.py:14-15,216-220, every yaml under configs/, lines 29-35
 *   kasf_adamw_step        <- optim.AdamW(...).step()             train_and_evaluate_sp.py:270-272,243
 *   kasf_gather_clips      <- Dataset.__getitem__ + DataLoader collate data/reader/sp_dataset.py:45-92
 *   kasf_joint_flip        <- joint_flip                            utils/utilities.py:128-135
 *   kasf_tta_merge         <- flip-TTA average + root zeroing        train_and_evaluate_sp.py:46-55
 *   kasf_eval_metrics      <- de-normalise + MPJPE/JPE/accel/P-MPJPE train_and_evaluate_sp.py:57-93, utils/error_calc.py:5-48
 *   kasf_lift_window_count <- turn_into_clips (number of clips)     demo/demo.py:132-156
 *   kasf_lift_windows      <- turn_into_clips + normalize_screen_coordinates + flip_data  demo/demo.py:132-156,222-227, demo/lib/utils.py:5-20
 *   kasf_lift_stitch       <- flip-TTA average + root zeroing + downsample of the tail clip  demo/demo.py:229-236
 *   kasf_lift_ragged_plan, kasf_lift_windows_ragged, kasf_lift_stitch_ragged <- the same three over many tracks of different lengths in one batch
 *   kasf_stream_tables, kasf_stream_push, kasf_stream_windows, kasf_stream_emit <- the same lift one frame at a time: per-player history on the device,
 *                             its last T frames (fewer: the demo's one resampled clip) lifted every tick            demo/demo.py:132-156,222-236
 *   kasf_coco_h36m         <- h36m_coco_format / coco_h36m (COCO-17 detector keypoints -> H36M-17)  demo/lib/preprocess.py:10-69, demo/demo.py:75-78
 *   kasf_pose_world        <- camera_to_world / qrot, feet on the floor, unit scale                demo/lib/utils.py:55-73, demo/demo.py:242-248
 *   kasf_heatmap_keypoints <- get_final_preds (get_max_preds, POST_PROCESS, transform_preds) and box_to_center_scale: what the demo does on the host between
 *                             HRNet's output tensor and the COCO keypoints   demo/lib/hrnet/gen_kpts.py:158-161, demo/lib/hrnet/lib/utils/inference.py:21-82,
 *                             demo/lib/hrnet/lib/utils/transforms.py:50-101, demo/lib/hrnet/lib/utils/utilitys.py:102-135
 *   kasf_heatmap_flip_keypoints <- the same behind HRNet's flip test: flip_back with the left / right pairs, SHIFT_HEATMAP, the float32 average
 *                             demo/lib/hrnet/lib/utils/transforms.py:15-30, demo/lib/hrnet/experiments/w48_384x288_adam_lr1e-3.yaml:119-121
 *   kasf_heatmap_decode    <- the same two decodes with DARK (Zhang et al., CVPR 2020; mmpose post_process = 'unbiased') or DARK-UDP (Huang et al., CVPR
 *                             2020; mmpose post_dark_udp, ViTPose) sub-pixel refinement and the UDP W - 1 / H - 1 affine; not in the demo, whose HRNet uses neither
 *   kasf_detect_boxes      <- predict_transform, write_results (objectness threshold, class arg-max, persons only, sort, greedy NMS) and the un-letterbox of
 *                             yolo_human_det: what the demo does between the YOLOv3 network's output and the person boxes
 *                             demo/lib/yolov3/util.py:34-81,107-225, demo/lib/yolov3/bbox.py:51-78, demo/lib/yolov3/human_detector.py:116-168
 *   kasf_crop_persons      <- PreProcess: box_to_center_scale, get_affine_transform, cv2.warpAffine, ToTensor, Normalize and the [2, 1, 0] channel swap: what the
 *                             demo does on the host between the person boxes and HRNet's input tensor
 *                             demo/lib/hrnet/lib/utils/utilitys.py:139-169, demo/lib/hrnet/gen_kpts.py:152-157, demo/lib/hrnet/lib/utils/transforms.py:58-101
 *   kasf_letterbox_plan, kasf_letterbox_frames <- prep_image: letterbox_image (cv2.resize INTER_CUBIC onto a canvas of 128), the [:, :, ::-1] channel reversal,
 *                             transpose and float().div(255.0): what the demo does on the host between a video frame and the YOLOv3 network's input
 *                             demo/lib/yolov3/preprocess.py:9-38, demo/lib/yolov3/human_detector.py:131
 *   kasf_yuv420_to_bgr     <- cap.read(): the YUV 4:2:0 -> BGR conversion behind cv2.VideoCapture, which the demo leaves to the host; here from the decoder's
 *                             NV12 / I420 surface in device memory to the uint8 BGR frame the two entries above take
 *                             demo/lib/hrnet/gen_kpts.py:106,118
 *   kasf_draw_poses, kasf_bgr_to_nv12, kasf_pose_panel <- plot_on_frame's lines and dots, the score threshold of plot_keypoint / write, the 3-D plot's projection
 *                             and the frame cv2.VideoWriter takes; here painted on the device frame and written as the encoder's NV12 surface (exact geometry,
 *                             not cv2's rasteriser)   demo/demo.py:91-105,159-191,307-323, demo/lib/hrnet/lib/utils/utilitys.py:24-58
 *   kasf_sort_update       <- Sort.update (KalmanBoxTracker, associate_detections_to_trackers, iou) and, from gen_video_kpts, the empty-frame hold and the
 *                             num_person oldest tracks: what the demo does on the host between the person boxes and the crops
 *                             demo/lib/sort/sort.py:15-222, demo/lib/hrnet/gen_kpts.py:111-148
 *   kasf_stream_track_front, kasf_stream_track_emit <- the seam between the two: gen_video_kpts hands each tracked person's keypoints to the lift by track
 *                             order; here the tracker's ids and slots drive the lifter's per-player histories on the device   demo/lib/hrnet/gen_kpts.py:125-170
 *   kasf_one_euro_push, kasf_one_euro_tracked, kasf_one_euro_tracks <- nothing in the reference (its unused revise_kpts, demo/lib/preprocess.py:72-103, patches
 *                             low-score leg joints): the One-Euro filter live pose pipelines put between the pose network and the lift, and behind the lift
 *   kasf_tracks_refine     <- nothing in the reference: what offline pose tooling puts in front of the lift for a file, interpolation across occlusion gaps and
 *                             a symmetric, zero-phase smoother
 *   kasf_bone_median, kasf_bone_apply, kasf_bone_push, kasf_bone_tracked <- nothing in the demo; the bone table is get_limb_lens' (utils/loss_calc.py) and the
 *                             quantity held constant is what loss_limb_var_calc penalises in training: one length per bone per player, re-imposed on every frame
 *   kasf_pose_place        <- nothing in the reference (its demo plots one person at the origin): the root translation that re-projects a root-relative pose
 *                             onto its keypoints through the camera's intrinsics, so that several players stand where they stood
 *   kasf_keypoints_triangulate, kasf_keypoints_undistort <- nothing in the reference (it is monocular): the keypoints of one player in several calibrated cameras
 *                             to joints in the world frame, and the Brown-Conrady undistortion that this and kasf_pose_place need in front of them
 *   kasf_match_pair_costs, kasf_match_groups <- nothing in the reference: which of the rows that several cameras' trackers emit are the same player, from the
 *                             gaps between their keypoints' rays; what puts kasf_keypoints_triangulate behind kasf_sort_update without a host round trip
 *   kasf_op_*              <- the individual nn.Modules under model/modules/ (unit-test entry points)
 *   kasf_op_gcn_fwd, kasf_op_gcn_bwd <- GCN.forward between its U | V Linear and the residual, and autograd of it   model/modules/graph.py:19-134, KASportsFormer.py:109
 */
#ifndef KASF_H_
#define KASF_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KASF_DTYPE_F32 0   /* parity mode: fp32 storage, exact-f32 MFMA (v_mfma_f32_16x16x4_f32) */
#define KASF_DTYPE_BF16 1  /* fast mode: bf16 activations/weights, fp32 accumulate/statistics/master weights */

#define KASF_FLAG_TRAIN 1       /* BatchNorm batch statistics + running-stat update; keep activations for backward */
#define KASF_FLAG_RETURN_REP 2  /* out is the [B,T,17,512] tanh representation (forward(x, return_rep=True)) */
#define KASF_FLAG_KEEP 4        /* keep activations for kasf_backward WITHOUT batch statistics: autograd through model.eval() (BatchNorm on running stats) */
#define KASF_FLAG_INPUT_GRAD 8  /* with TRAIN or KEEP: kasf_backward also leaves d/dx [B,T,17,3] fp32 in the workspace entry "dx_input" (x.requires_grad_()) */

typedef struct kasf_model kasf_model;

typedef struct kasf_config {
    int32_t n_layers;            /* 26 in the shipped yaml (configs/sportspose-gt-kasportsformer.yaml:71) */
    int32_t n_frames;            /* T in [4, 256]: sizes the temporal BatchNorm1d; 9 / 27 / 81 have tuned temporal kernels, T <= 96 MFMA attention cores */
    int32_t num_heads;           /* 8 in every yaml (:84; head dim 16: MFMA attention kernels); 2 / 4 / 16 run generic kernels (4 = the constructor's default; 2: n_frames <= 157) */
    int32_t neighbour_num;       /* top-k of the temporal GCN adjacency (graph.py:104-112), 1..4; every yaml uses 4 (:89); other values are rejected */
    int32_t use_adaptive_fusion; /* 1: softmax gate, 0: plain mean (KASportsFormer.py:284) */
    int32_t dtype;               /* KASF_DTYPE_* */
} kasf_config;

const char* kasf_last_error(void);
/* Process-wide: 1 = the three branches of a layer run back to back on the caller's stream instead of on three streams (the mode isolated kernel
 * profiles are taken in; it costs a quarter of the training throughput since round 4: the MLP launches of the engine take half the chip -- so that two
 * branches' launches run side by side -- and the grids are the same in both settings, for the sake of the bits).  NOT a determinism switch: gradients are reproducible from run to run either way and
 * the two settings give the same bits (every gradient reduction is a fixed-order sum; the BatchNorm batch statistics, which cross workgroups through
 * atomics, are accumulated EXACTLY -- 52-bit pieces of a fixed-point number, 64-bit integer atomic adds, csrc/k_gcn.hip -- so their totals do not depend on
 * arrival order either: since ABI 7 there is no exception left).  Default 0 (or 1 when KASF_SINGLE_STREAM is set in the environment).
 * kasf_forward / kasf_backward read the setting once per call.  kasf_set_deterministic / kasf_get_deterministic are the round-3 names of the same
 * two functions, kept as aliases. */
void kasf_set_single_stream(int32_t on);
int32_t kasf_get_single_stream(void);
/* Process-wide: from how many tokens per launch (M = batch x frames x 17) the bf16 backward forms the mixers' weight gradients INSIDE the data-gradient kernels
 * (one bf16 partial tile per workgroup, fixed-order reduce) instead of in a separate streaming launch.  Default 40,000 (below it the partial tiles cost more
 * than the second pass over dY they save); tokens < 0 restores the default.  Both forms are bit-reproducible; they differ from each other at bf16 rounding
 * level (tests/test_gpu_determinism.py compares them on one shape). */
void kasf_set_fused_wgrad_min_tokens(int64_t tokens);
int64_t kasf_get_fused_wgrad_min_tokens(void);
/* Process-wide (ABI 8), OPT-IN: 1 (default 0; 1 when KASF_ATTN_BWD_FUSED=1 is in the environment) = in bf16 mode with 8 heads the backward of an attention / bone block whose
 * groups have at most 32 positions (every spatial block; temporal blocks up to n_frames = 32) is ONE launch that re-forms LN(x), q | k | v and the attention output from the
 * block input (csrc/k_attn_bwd_f.hip; reference: modules/selfattention.py:18-57, modules/bone_crossattention.py:19-62, KASportsFormer.py:103-110) followed by one streaming
 * weight-gradient launch: the training forward then saves no q | k | v | o for these blocks and kasf_workspace_bytes shrinks accordingly (T = 27, B = 256: 26.9 -> 14.4 GB).
 * 0 = the four-launch sequence (saved q | k | v | o, attention cores, data gradient + LayerNorm backward with the fused weight gradient, proj weight gradient): 15 % FASTER per
 * training step on MI355X, hence the default.  Both are bit-reproducible; they agree with each other at bf16 rounding level
 * (tests/test_gpu_determinism.py).  kasf_workspace_bytes, kasf_forward and kasf_backward of one step must see the SAME setting (the workspace layout and what the forward saves
 * depend on it): change it only between steps, then re-query kasf_workspace_bytes.  on < 0 restores the default.  `on` is a bit mask of block kinds -- 1 self-attention
 * spatial, 2 self-attention temporal, 4 bone spatial, 8 bone temporal; on = 1 means all four (15), which is also what kasf_get_fused_attn_bwd then returns.  Measured in the
 * three-stream step (B = 256, T = 27): mask 2 runs at the default's speed (4,625-4,646 against 4,635-4,660 clips/s) with 7 GB less HBM traffic per step; 3: -2 %; 10: -5 %. */
void kasf_set_fused_attn_bwd(int32_t on);
int32_t kasf_get_fused_attn_bwd(void);
void kasf_set_deterministic(int32_t on);
int32_t kasf_get_deterministic(void);
int kasf_version(void);

/* Streams: every model forks its attention / graph / bone branches onto ONE process-wide pair of side streams per device (created with the first model of
 * the device, released with the process; device indices 0..63, error 2 beyond).  Events order every fork and join, so any number of models may share the
 * pair; models of one device driven from different host threads therefore serialise on it, and a stream capture of kasf_forward has to be the only work
 * in flight on that device while it is recorded. */
int kasf_model_create(const kasf_config* cfg, kasf_model** out);
/* the same handle without touching a device: answers every layout / size query below (kasf_param_*, kasf_buffer_*, kasf_workspace_bytes, kasf_stage_grad_range ...);
 * what a host-side binding uses to build its module tree before any GPU exists (kasportsformer_amd/model.py does) */
int kasf_model_create_layout_only(const kasf_config* cfg, kasf_model** out);
void kasf_model_destroy(kasf_model* m);

/* 0 = healthy.  Non-zero: a kernel's bounded wait on another workgroup ran out (the affected gradient rows were poisoned with NaN instead of
 * hanging the GPU); blocking device read -- for tests and post-mortems, not for the step loop. */
int kasf_model_status(const kasf_model* m, int32_t* status);

/* ---- parameter / buffer layout: one flat fp32 array each; entries carry the reference's state_dict names ---- */
int64_t kasf_param_count(const kasf_model* m);       /* elements of the flat parameter (and gradient) array, multiple of 4 */
int64_t kasf_param_live_count(const kasf_model* m);  /* [0, live) receive gradients; [live, count) are the never-used norm1_limb */
int32_t kasf_param_entries(const kasf_model* m);
int kasf_param_entry(const kasf_model* m, int32_t idx, char* name, int32_t name_cap, int64_t* offset, int32_t* ndim, int64_t shape[4]);
int64_t kasf_buffer_count(const kasf_model* m);      /* BatchNorm running_mean / running_var, fp32 */
int32_t kasf_buffer_entries(const kasf_model* m);
int kasf_buffer_entry(const kasf_model* m, int32_t idx, char* name, int32_t name_cap, int64_t* offset, int32_t* ndim, int64_t shape[4]);
/* gradient ranges that become final after each backward stage (data-parallel all-reduce buckets) */
int32_t kasf_backward_stages(const kasf_model* m);   /* n_layers + 2: head, layers (last to first), prologue */
int kasf_stage_grad_range(const kasf_model* m, int32_t stage, int64_t* begin, int64_t* end);

/* ---- kernel-side weight arena (dtype of the model; transposed / layer-scale-folded copies) ---- */
int64_t kasf_packed_bytes(const kasf_model* m);
int kasf_pack_weights(const kasf_model* m, const float* params, void* packed, void* stream);

/* ---- workspace (activations kept for backward + scratch); caller allocates, 256-B aligned ---- */
int64_t kasf_workspace_bytes(const kasf_model* m, int32_t batch, int32_t flags);

/* x [B,T,17,3] fp32 -> out [B,T,17,3] fp32 (or [B,T,17,512] with KASF_FLAG_RETURN_REP).
 * `buffers` (BN running stats) is updated when KASF_FLAG_TRAIN is set.  x and out must not alias.
 * batch >= 1 and batch * n_frames * 17 * 384 < 2^31 (the kernels address activations with 32-bit element offsets): error 2 otherwise. */
int kasf_forward(const kasf_model* m, const float* params, const void* packed, float* buffers, const float* x, float* out, void* workspace,
                 int64_t workspace_bytes, int32_t batch, int32_t flags, void* stream);

/* Gradients of a preceding kasf_forward(KASF_FLAG_TRAIN or KASF_FLAG_KEEP) on the same workspace; `flags` = the forward's flags:
 * KASF_FLAG_TRAIN selects the batch-statistics BatchNorm backward (otherwise running statistics are constants), KASF_FLAG_RETURN_REP means
 * dout is the gradient of the [B,T,17,512] representation (otherwise dout [B,T,17,3] fp32).
 * KASF_FLAG_INPUT_GRAD (pass it to kasf_workspace_bytes, kasf_forward, kasf_backward and kasf_ws_entry alike; it has no effect without TRAIN or KEEP): the
 * workspace ends in three more fp32 [B*T*17*3] entries, "dx_joint3", "dbone3" and "dx_input"; the last stage writes the gradient with respect to x into
 * "dx_input" (kasf_op_input_grad's arithmetic on the input gradients of the three embeddings; found by name through kasf_ws_entry, valid once the last stage
 * has run, bit-reproducible, once-differentiable).  Without the flag the plan, the launches and every result are what they are without it.
 * Accumulates (+=) into grads[0, live); the caller zeroes it.  Stages [stage_begin, stage_end) of
 * kasf_backward_stages() are run; call with (0, stages) for the whole backward, or stage by stage to
 * overlap the gradient all-reduce of finished ranges. */
int kasf_backward(const kasf_model* m, const float* params, const void* packed, const float* dout, float* grads, void* workspace,
                  int64_t workspace_bytes, int32_t batch, int32_t flags, int32_t stage_begin, int32_t stage_end, void* stream);

/* losses: `losses_floats` >= 4 + 4 * batch floats (error 5 otherwise: the capacity is an argument since ABI 6, so that a caller written against the
 * 4-float buffer of ABI <= 4 fails to compile instead of being overrun); on return losses[0..3] = {total, mpjpe, n_mpjpe, velocity} (the rest is
 * scratch: per-clip sums, added in a fixed order so that the result is bit-reproducible); dpred = grad_scale * dTotal/dpred */
int kasf_loss3(const float* pred, const float* target, float* dpred, float* losses, int64_t losses_floats, int32_t batch, int32_t n_frames,
               float lambda_n_mpjpe, float lambda_velocity, float grad_scale, void* stream);

/* The reference's complete loss (train_and_evaluate_sp.py:216-220, `loss_total_complete`) and its gradient, one launch per call plus the fixed-order finish.
 * `lambdas`: six HOST floats {n_mpjpe, velocity, limb_len_var, limb_len, limb_cos_simi, limb_cos_simi_velocity}, the yaml keys lambda_n_mpjpe,
 * lambda_mpjpe_velocity, lambda_limb_len_var, lambda_limb_len, lambda_limb_cos_simi, lambda_limb_cos_simi_velocity (every yaml under configs/, lines 29-35), read before return.
 * On return losses[0..7] = {total, mpjpe, n_mpjpe, velocity, limb_len_var, limb_len, cos_simi, cos_simi_velocity}; all seven parts are computed whatever the
 * lambdas are (the reference logs them).  Behind them the per-clip sums, losses[8 + 8 * b + k] for part k + 1 (k = 7 unused), added in a fixed order:
 * `losses_floats` >= 8 + 8 * batch (error 5 otherwise); batch, n_frames >= 1 and n_frames <= KASF_LOSS7_MAX_FRAMES (error 2).  dpred = grad_scale * dTotal/dpred.
 *   limbs    l_k = x[a_k] - x[b_k] for the 16 pairs of get_limb_lens (utils/loss_calc.py:33-41), len_k = |l_k|
 *   angles   the 18 limb pairs (i, j) of get_limb_cos_simi (loss_calc.py:69-78): c = (l_i / max(|l_i|, 1e-8)) . (l_j / max(|l_j|, 1e-8)) (torch 2.x
 *            cosine_similarity), theta = acos(clamp(c, -1 + 1e-7, 1 - 1e-7)), the two bounds rounded to fp32
 *   limb_len_var       mean over (B, 16) of the unbiased variance over t of len_pred; 0 when n_frames <= 1            loss_calc.py:45-51
 *   limb_len           mean over (B, T, 16) of |len_pred - len_target|                                               loss_calc.py:54-58
 *   cos_simi           mean over (B, T, 18) of |theta_pred - theta_target|                                           loss_calc.py:80-83
 *   cos_simi_velocity  mean over (B, T - 1, 18) of |(theta_p[t+1] - theta_p[t]) - (theta_y[t+1] - theta_y[t])|; 0 when n_frames <= 1   loss_calc.py:86-94
 * Gradients follow torch: sign(0) = 0 for the L1 terms, nothing through clamp outside its closed range, nothing through a norm at the zero vector (a zero-length
 * limb gives theta = pi / 2 and a finite gradient).  fp32, no atomics, every sum in a fixed order: values and dpred are bit-reproducible from run to run, and a
 * clip's dpred rows and per-clip sums do not depend on the other clips of the batch beyond `batch` itself.  The three old terms are computed exactly as
 * kasf_loss3 computes them and a term whose lambda is 0.f adds nothing to dpred: with the four new lambdas zero, dpred and losses[0..3] are kasf_loss3's bits. */
#define KASF_LOSS7_MAX_FRAMES 360
int kasf_loss7(const float* pred, const float* target, float* dpred, float* losses, int64_t losses_floats, int32_t batch, int32_t n_frames,
               const float* lambdas /* host, 6 floats: n_mpjpe, velocity, limb_len_var, limb_len, limb_cos_simi, limb_cos_simi_velocity */, float grad_scale,
               void* stream);

/* torch.optim.AdamW step over n contiguous fp32 elements (n multiple of 4); step_index starts at 1 */
int kasf_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int32_t step_index, float grad_scale, void* stream);

/* ---- AdamW over a LIST of element ranges of the flat arrays, and the global norm of the gradient over the same list (ABI 12 additions; what
 * kasportsformer_amd.AdamW, a torch.optim.AdamW subclass with parameter groups, parameter subsets, per-parameter step counts and norm clipping, launches) ----
 * The caller describes the elements to update by a CHUNK TABLE in device memory, `n_chunks` records of 16 bytes:
 *   begin   element index into params / grads / exp_avg / exp_avg_sq (all four are indexed alike), any value >= 0
 *   count   1 .. KASF_OPT_CHUNK_MAX elements; begin + count <= n
 *   cls     0 .. n_classes - 1: whose hyper-parameters the chunk's elements take (ignored by kasf_grad_norm)
 * The caller builds it: take every parameter that steps as a segment (offset, numel, class), merge segments that touch and share a class into runs, cut every
 * run into pieces of at most KASF_OPT_CHUNK_MAX elements (kasportsformer_amd/optim.py: plan_chunks does exactly this).  Chunks must not overlap; their order is free
 * for the update and fixes the summation order of the norm.  begin and count need no alignment: a chunk's elements before the first and behind the last 16-byte
 * boundary go through scalar accesses.  Elements outside every chunk are neither read-modified nor written, in any of the arrays.  The four array bases, like
 * kasf_adamw_step's, must be 16-byte aligned. */
#define KASF_OPT_CHUNK_MAX 4096
#define KASF_OPT_MAX_CLASSES 32
typedef struct KasfOptChunk {
    int64_t begin;
    int32_t count;
    int32_t cls;
} KasfOptChunk;
typedef struct KasfAdamwClass {
    float lr, beta1, beta2, eps, weight_decay;
    float bc1, bc2;      /* OUT of the caller's hands: kasf_adamw_segments forms 1 - beta^step in double from `step` below, as kasf_adamw_step does */
    int32_t step;        /* >= 1: the step count, after its increment, of every parameter of the class */
} KasfAdamwClass;
typedef struct KasfAdamwClasses {
    KasfAdamwClass c[KASF_OPT_MAX_CLASSES];
} KasfAdamwClasses;

/* One launch: for every element i of every chunk, with its class's values, kasf_adamw_step's statements with `grad_scale` replaced by
 * s = clip ? grad_scale * clip[1] : grad_scale (one fp32 product); `clip` is kasf_grad_norm's out2 or NULL.  `classes`: n_classes HOST records, 1..32 (a caller with
 * more splits its table into several calls), passed to the kernel by value, so changing a learning rate needs no upload.  With clip == NULL, one class and one
 * chunked run [0, n), n a multiple of 4, the result has kasf_adamw_step's bits.  n_chunks == 0: nothing happens.
 * Errors: 2 for a null pointer (chunks may be NULL only with n_chunks == 0), misaligned array, n < 0, n_chunks < 0, n_classes outside 1..32, a class step < 1. */
int kasf_adamw_segments(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const KasfOptChunk* chunks /* device */, int64_t n_chunks,
                        const KasfAdamwClass* classes /* host */, int32_t n_classes, float grad_scale, const float* clip /* device, 2 floats, nullable */,
                        void* stream);

/* Two launches: out2[0] = (float)(sqrt(sum over the chunks' elements of (double)g * (double)g) * (double)grad_scale) -- with grad_scale = 1 / world_size the norm
 * of the averaged gradient -- and out2[1] = min(1.0f, max_norm / (out2[0] + 1e-6f)), torch.nn.utils.clip_grad_norm_'s coefficient (a NaN norm gives a NaN
 * coefficient as it does there; max_norm = +inf measures without clipping: 1.0f exactly for a finite norm).  `partial`: n_chunks doubles of device scratch, one
 * per chunk, each summed in an order that its chunk's (begin, count) alone fix, then added in index order through a fixed tree by one workgroup: no atomics, the
 * same bits from run to run and for every grid width.  n_chunks == 0: nothing happens (out2 keeps its contents).
 * Errors: 2 for a null pointer, a misaligned grads, n < 0, n_chunks < 0. */
int kasf_grad_norm(const float* grads, int64_t n, const KasfOptChunk* chunks /* device */, int64_t n_chunks, double* partial /* device */, float grad_scale,
                   float max_norm, float* out2 /* device, 2 floats */, void* stream);

/* ---- batch assembly from a clip set resident in device memory: x_all/y_all [n_clips,T,17,3] fp32 (y_all may be NULL) ----
 * x_out[b] = x_all[index[b]] (same for y), left/right flipped (flip_data, sp_dataset.py:36-40) where flip[b] != 0 (flip may be NULL).
 * An index outside [0,n_clips) yields a zero clip. */
int kasf_gather_clips(const float* x_all, const float* y_all, const int64_t* index, const uint8_t* flip, int64_t n_clips, int32_t batch,
                      int32_t n_frames, float* x_out, float* y_out, void* stream);

/* ---- evaluation side: fp32 [rows = B*T][17][3] poses ---- */
/* dst = joint_flip(src): x negated, left joints [1,2,3,14,15,16] swapped with right [4,5,6,11,12,13]; src != dst */
int kasf_joint_flip(const float* src, float* dst, int64_t rows, void* stream);
/* out = (pred + joint_flip(pred_of_flipped)) / 2 with the root joint zeroed; pred_of_flipped == NULL: root zeroing only */
int kasf_tta_merge(const float* pred, const float* pred_of_flipped, float* out, int64_t rows, void* stream);
/* The reference's per-clip evaluation loop in one launch.  pred [B,T,17,3] (normalised model output, root zeroed here again),
 * label_scaled [B,T,17,3] (mm), factor [B,T], res [B,2] = (w,h) as floats, action [B] ids in [0,n_actions) (or NULL with action_sums NULL).
 * Per-frame outputs: mpjpe [B,T], p_mpjpe [B,T], accel [B,T-2], jpe [B,T,17].  action_sums [n_actions][KASF_EVAL_COLS] fp64 is
 * ACCUMULATED into: columns = sum mpjpe, sum p_mpjpe, sum accel, sum jpe[17], #frames, #accel frames. */
#define KASF_EVAL_COLS 22
int kasf_eval_metrics(const float* pred, const float* label_scaled, const float* factor, const float* res, const int32_t* action, int32_t batch,
                      int32_t n_frames, int32_t n_actions, float* mpjpe, float* p_mpjpe, float* accel, float* jpe, double* action_sums, void* stream);

/* ---- lifting a 2-D keypoint track to 3-D poses (demo/demo.py:194-254, lift_3d_pose): track [P][n][17][3] fp32 = pixel x, y, confidence ----
 * The window plan: W windows of T frames (T in [1, 256], stride in [1, T]).
 *   stride == T (the demo): windows start at 0, T, 2T, ...; a last window of L < T frames (and the one window of a track with n < T) is resampled
 *     to T frames through resample[T] = demo.py:132-136's resample(L, T), computed on the host (float64 linspace, floor, clip).  n = k * T gives
 *     k full windows (turn_into_clips, demo.py:138-156, raises UnboundLocalError there).
 *   stride < T (not in the demo): n <= T as above; otherwise windows start at 0, stride, 2 * stride, ... while start + T < n, plus one at n - T,
 *     all full, and each frame's output is the mean over the windows that cover it (summed in ascending window order, then divided).
 * kasf_lift_window_count returns W (0 for n = 0), or a negative error code with kasf_last_error() set; it needs no device. */
int64_t kasf_lift_window_count(int64_t n, int32_t T, int32_t stride);
/* x_out [(1 + flip) * persons * W][T][17][3]: clip (h * persons + p) * W + w is window w of person p, h = 1 the mirrored copy (the stacking of
 * predict_flip_tta).  Each frame is normalised as normalize_screen_coordinates (demo/lib/utils.py:16-20): fp32 x / width * 2, then an fp64
 * subtraction of [1, height / width], stored as fp32; the confidence passes through.  The mirrored copy applies flip_data (demo/lib/utils.py:5-13:
 * x negated, left joints [1,2,3,14,15,16] swapped with right [4,5,6,11,12,13]) to a copy: the track is never written (demo.py:227 flips its
 * input in place, so both of its forwards see the mirrored clip).  resample [T] (device) is required when the plan has a resampled window, else
 * ignored (may be NULL). */
int kasf_lift_windows(const float* track, int32_t persons, int64_t n, float width, float height, int32_t T, int32_t stride, const int32_t* resample,
                      int32_t flip, float* x_out, void* stream);
/* out [persons][n][17][3] from the model's output pred [(1 + flip) * persons * W][T][17][3]: per window (pred + joint_flip(pred of the mirrored
 * copy)) / 2 (flip = 0: pred alone), root joint zeroed -- kasf_tta_merge's arithmetic, demo.py:229-235 -- and scattered back to the track: frame
 * start + j of the resampled window reads position first_pos[j], the first t with resample[t] == j (demo.py:146-153's downsample,
 * np.unique(r, return_index=True)[1]).  first_pos [L] (device) is required when the plan has a resampled window, else ignored (may be NULL). */
int kasf_lift_stitch(const float* pred, int32_t flip, int32_t persons, int64_t n, int32_t T, int32_t stride, const int32_t* first_pos, float* out,
                     void* stream);

/* ---- many tracks of different lengths in one call (ABI 10; one track per tracked person, each its own length) ----
 * Packed layout: the tracks back to back in packed [frames][17][3] fp32; track p is rows offsets[p] .. offsets[p + 1] - 1, offsets [tracks + 1]
 * int64 with offsets[0] = 0 and offsets[tracks] = frames.  Each track is cut by its own plan (the rule above with its own n; one T and one stride
 * for the call), and win_first [tracks + 1] int64 is the prefix sum of the per-track window counts: track p owns windows win_first[p] ..
 * win_first[p + 1] - 1, win_first[tracks] = windows.
 * kasf_lift_ragged_plan fills win_first from the track lengths (host arrays; it needs no device) and returns windows, or a negative error code with
 * kasf_last_error() set (bad T or stride, tracks < 0, a negative length), in which case nothing is written. */
int64_t kasf_lift_ragged_plan(const int64_t* lengths, int32_t tracks, int32_t T, int32_t stride, int64_t* win_first);
/* x_out [(1 + flip) * windows][T][17][3]: clip h * windows + win_first[p] + w is window w of track p, h = 1 the mirrored copy (equal lengths: the
 * clip order of kasf_lift_windows, (h * persons + p) * W + w).  Track p is normalised with its own width[p] and height[p] (device fp32 [tracks],
 * positive), bit for bit what kasf_lift_windows writes for that track alone.  resample [tracks][T] int32 (device): row p is the track's resample
 * table when its plan has a resampled window and is not read otherwise. */
int kasf_lift_windows_ragged(const float* packed, const int64_t* offsets, const int64_t* win_first, int32_t tracks, int64_t frames, int64_t windows,
                             const float* width, const float* height, int32_t T, int32_t stride, const int32_t* resample, int32_t flip, float* x_out,
                             void* stream);
/* out [frames][17][3] from the model's output pred [(1 + flip) * windows][T][17][3] in the clip order above: kasf_lift_stitch's arithmetic per
 * track.  first_pos [tracks][T] int32 (device): row p holds the track's first_pos in its first L entries when its plan has a resampled window
 * and is not read otherwise.
 * Both entries: offsets, win_first, width, height and the tables are device arrays that are only read, and required whenever windows > 0;
 * tracks, frames and windows are the host's copies of the sizes (error 2 when they cannot belong to one plan).  Every index formed from a device
 * table is clamped into the arrays those sizes describe: an inconsistent table gives wrong poses, never an access outside the arrays. */
int kasf_lift_stitch_ragged(const float* pred, int32_t flip, const int64_t* offsets, const int64_t* win_first, int32_t tracks, int64_t frames,
                            int64_t windows, int32_t T, int32_t stride, const int32_t* first_pos, float* out, void* stream);

/* ---- one new frame per tick (ABI 11): the online form of the lift, per-player history that stays on the device ----
 * A slot holds one player's recent frames: ring [S][T][17][3] fp32 raw pixel keypoints (frame number c of a slot at ring position c % T) and count [S]
 * int64, the frames pushed since the slot's reset (a reset is zeroing the count entry; the ring needs no clearing).  A slot's current window is its last
 * L = min(count, T) frames; a window of L < T frames is lifted as the demo lifts a track shorter than one clip (turn_into_clips, demo/demo.py:138-156: the
 * one clip resampled to T frames), a full one as one clip.  The plans of all L are two host-built tables [T + 1][T] int32, so nothing is planned per tick:
 * kasf_stream_tables fills row n (1 <= n < T) of resample_tab with demo.py:132-136's resample(n, T) -- clamp(floor((double)t * ((double)n / (double)T)),
 * 0, n - 1), which is np.linspace(0, n, T, endpoint=False) floored and clipped -- and of first_pos_tab, in its first n entries (zeros after), with the first t of
 * every frame (demo.py:146-153's downsample, np.unique(r, return_index=True)[1]); row T is the identity 0 .. T - 1 in both, row 0 is zeros.  Host arrays, no
 * device needed; error 2 (T outside [1, 256], a null pointer) writes nothing. */
int kasf_stream_tables(int32_t T, int32_t* resample_tab, int32_t* first_pos_tab);
/* The three device entries share K (slots of this call), S (slots of the state), T and slots [K] int32 (device): distinct ids in [0, S), or NULL for
 * "slot i for row i", which needs K == S.  Error 2: T outside [1, 256], K or S negative, K > S, NULL slots with 0 < K < S, a required pointer that is
 * null.  K = 0 does nothing.  ring, count, width, height and the tables are device arrays; only kasf_stream_push writes ring and count.  Every index formed
 * from a device array (slot id, count, table entry) is clamped into the arrays S and T describe, and a count below 1 is read as 1: an inconsistent state
 * gives wrong poses, never an access outside the arrays.
 * kasf_stream_push stores row i of frames [K][17][3] at ring[slot][count[slot] % T], then count[slot] += 1. */
int kasf_stream_push(const float* frames, const int32_t* slots, int32_t K, int32_t S, int32_t T, float* ring, int64_t* count, void* stream);
/* x_out [(1 + flip) * K][T][17][3]: clip h * K + i is the current window of slot i of the call, h = 1 the mirrored copy (the stacking of
 * predict_flip_tta).  Clip frame t of a slot with count k is ring position (k - L + resample_tab[L][t]) % T, normalised with the slot's width[slot] and
 * height[slot] (device fp32 [S], positive) and mirrored bit for bit as kasf_lift_windows_ragged does it (normalize_screen_coordinates and flip_data,
 * demo/lib/utils.py:5-20; demo.py:222-227). */
int kasf_stream_windows(const float* ring, const int64_t* count, const int32_t* slots, int32_t K, int32_t S, int32_t T, const float* width,
                        const float* height, const int32_t* resample_tab, int32_t flip, float* x_out, void* stream);
/* out [K][n_out][17][3] from the model's output pred [(1 + flip) * K][T][17][3] in the clip order above: row r of slot i is window frame
 * j = clamp(L - 1 - back + r, 0, L - 1), read at clip position first_pos_tab[L][j] and merged as kasf_lift_stitch merges a frame of one window
 * ((pred + joint_flip(pred of the mirrored copy)) / 2, flip = 0: pred alone; root joint zeroed; demo.py:229-236).  back in [0, T - 1], n_out in [0, T]
 * (0 does nothing).  back = D, n_out = 1 is the pose D frames behind the newest one; back = D - 1, n_out = D the D newest frames at the end of a track. */
int kasf_stream_emit(const float* pred, int32_t flip, const int64_t* count, const int32_t* slots, int32_t K, int32_t S, int32_t T,
                     const int32_t* first_pos_tab, int32_t back, int32_t n_out, float* out, void* stream);

/* ---- the two ends of the lift that the demo does on the host (new symbols of ABI 11; frames of [17][3] fp32 on the device) ----
 * kasf_coco_h36m: coco [frames][17][3] = pixel x, pixel y, score in COCO joint order (what YOLO-pose, RTMPose, ViTPose and the demo's HRNet emit) ->
 * h36m [frames][17][3] in the Human3.6M order the model was trained on.  Coordinates as coco_h36m (demo/lib/preprocess.py:10-37, the file the demo
 * imports: spine factor 2), statement by statement in fp32 -- the neck correction reads the copied nose, the spine x correction the pelvis and the thorax
 * before the thorax y correction -- and scores as h36m_coco_format (preprocess.py:58-62): bit for bit the reference's values.  Shapes are kept: a frame
 * of zeros gives a frame of zeros (the reference drops a whole person whose coordinates sum to exactly zero; its valid_frames and the unused
 * revise_kpts are not reproduced).  coco and h36m must not overlap.  frames = 0 does nothing; error 2 for frames < 0, or a null pointer with frames > 0
 * (no device needed to refuse). */
int kasf_coco_h36m(const float* coco, int64_t frames, float* h36m, void* stream);
/* kasf_pose_world: poses [frames][17][3] camera space (the lift's output) -> out [frames][17][3]: every joint v becomes v + 2 (q0 (q x v) + q x (q x v)) + t
 * with q = quat4[1..3], in fp32 and in qrot's operation order (demo/lib/utils.py:55-73); with `floor` the frame's smallest z is then subtracted from
 * its z column (demo.py:246), and with `unit` all 51 values are then divided by their largest (demo.py:247-248; a frame whose largest value is 0 gets
 * the reference's division by zero, unguarded).  quat4 (w, x, y, z) and trans3 are HOST pointers to 4 and 3 floats, read during the call and passed by
 * value into the launch; trans3 = NULL means zero (the demo's t = 0).  poses and out must not overlap.  frames = 0 does nothing; error 2 for
 * frames < 0, or a null poses / quat4 / out with frames > 0 (no device needed to refuse). */
int kasf_pose_world(const float* poses, int64_t frames, const float* quat4, const float* trans3, int32_t floor, int32_t unit, float* out, void* stream);

/* ---- pose-network heatmaps -> keypoints (a symbol ADDED under ABI 12: no existing entry changed, so the number did not; look it up by name) ----
 * hm [n][17][H][W], contiguous, of KASF_DTYPE_F32, KASF_DTYPE_F16 or KASF_DTYPE_BF16 (the 16-bit types are widened to fp32 on load, which is exact; every rule
 * below is on the fp32 values) -> out [n][17][3] fp32 = image x, image y, score per joint: get_final_preds (inference.py:52-82) of a top-down pose network
 * (HRNet, ViTPose, SimpleBaseline), per map:
 *   argmax    score = the map's largest value, position = its FIRST occurrence in row-major order (np.argmax); a map with a NaN gives score NaN at the first
 *             NaN.  x = idx % W, y = idx / W; where "score > 0" is false (zero, negative, NaN) the position is (0, 0)                  (inference.py:21-49)
 *   refine    (refine != 0; the demo's TEST.POST_PROCESS) only where 1 < x < W - 1 and 1 < y < H - 1, strictly: x += 0.25 sign(hm[y][x + 1] - hm[y][x - 1]),
 *             the same for y; fp32 differences, sign(0) = 0, a NaN difference gives NaN                                                 (inference.py:59-72)
 *   to image  transform_preds with rot = 0: the anchors sw = fl32(scale_x * 200), s1y = fl32(cy - sw / 2), dy = fl32(cy - s1y), s2x = fl32(cx - dy) as the
 *             reference stores them, then in fp64 kx = (cx - s2x) / (W / 2), ky = (cy - s1y) / (W / 2), x_img = cx + (x - W / 2) kx, y_img = cy + (y - H / 2) ky,
 *             each rounded once to fp32.  Only scale_x enters and both axes divide by W / 2, as in the reference.  The reference solves the same three-point
 *             system with cv2.getAffineTransform and is within 1 fp32 ulp of this closed form                                    (transforms.py:50-101)
 * geom [n][4] fp32 (device), per person: KASF_GEOM_CENTER_SCALE = (cx, cy, scale_x, scale_y), the pair the crop was made with; KASF_GEOM_BOX = the detector's
 * box (x1, y1, x2, y2), from which center and scale are derived as box_to_center_scale does (utilitys.py:102-135): in fp64 on the widened box, the box grown to
 * width / height = `aspect`, divided by 200, stored as fp32, then * 1.25 in fp32 unless center x == -1.  `aspect` is a double because the demo passes
 * frame_height / frame_width evaluated in fp64 (utilitys.py:151: image.shape[0], image.shape[1]); pass what the crop was made with.  It is ignored with
 * KASF_GEOM_CENTER_SCALE.
 * out_layout: KASF_LAYOUT_COCO = the network's joint order; KASF_LAYOUT_H36M = kasf_coco_h36m of that result, bit for bit, as a second launch on the same stream:
 * coco_scratch [n][17][3] fp32 (device, not overlapping out) is then required and is left holding the COCO result; it is ignored (may be NULL) with KASF_LAYOUT_COCO.
 * hm and geom are only read.  n = 0 does nothing.  Error 2, before a device or a pointer is touched: n < 0, H or W < 1, H * W > 2^24 (the reference's index
 * arithmetic is fp32), an unknown dtype, geom_kind or out_layout, aspect <= 0 (or NaN) with KASF_GEOM_BOX, a required pointer that is null with n > 0. */
#define KASF_DTYPE_F16 2           /* IEEE half: heatmap / detector input and crop output only, no model runs in it */
#define KASF_GEOM_CENTER_SCALE 0
#define KASF_GEOM_BOX 1
#define KASF_LAYOUT_COCO 0
#define KASF_LAYOUT_H36M 1
int kasf_heatmap_keypoints(const void* hm, int32_t dtype, int64_t n, int32_t H, int32_t W, const float* geom, int32_t geom_kind, double aspect, int32_t refine,
                           int32_t out_layout, float* out, float* coco_scratch, void* stream);

/* ---- flip-tested pose-network heatmaps -> keypoints (a symbol ADDED under ABI 12: additive, kasf_version() stays 12; look it up by name) ----
 * The flip test of a top-down pose network (HRNet's TEST.FLIP_TEST with SHIFT_HEATMAP, w48_384x288_adam_lr1e-3.yaml:119-121; flip_back and its matched_parts,
 * transforms.py:15-30) merged and decoded in ONE launch: hm [n][17][H][W] is the network's output for the crops, hm_flipped [n][17][H][W] its output for the
 * mirrored crops (input.flip(3)), both of `dtype` (KASF_DTYPE_F32, _F16 or _BF16; the 16-bit types are widened to fp32 on load, which is exact), contiguous,
 * only read.  On the fp32 values:
 *   src_x(x)           = shift ? min(W - x, W - 1) : W - 1 - x
 *   merged[p][j][y][x] = (hm[p][j][y][x] + hm_flipped[p][partner[j]][y][src_x(x)]) * 0.5f
 * one fp32 add and one fp32 multiply, not contracted, denormals kept: (output + output_flipped) * 0.5 of float32 numpy arrays.  With `shift`, src_x is
 * output_flipped[:, :, :, 1:] = output_flipped.clone()[:, :, :, 0:-1] after flip_back: column 0 keeps its unshifted value, every other column takes its left
 * neighbour's; W = 1 falls under the same formula.  inf + (-inf) is a NaN like any other.  For 16-bit input this is NOT what half-precision arithmetic on the
 * tensors would give: it is the reference's float32 procedure applied to the exact upcasts.
 * merged is then decoded exactly as kasf_heatmap_keypoints decodes a map -- first maximum in row-major order, first NaN wins and scores NaN, the "score > 0"
 * mask, the quarter-pixel refinement with strict bounds and fp32 differences of MERGED neighbours, the crop geometry, the fp64 affine -- into out [n][17][3].
 * partner: a HOST array of 17 joint indices, read during the call and passed by value into the launch; NULL = the COCO pairs (1,2) (3,4) (5,6) (7,8) (9,10)
 * (11,12) (13,14) (15,16), joint 0 its own partner.  It must be an involution on 0..16: every value in range and partner[partner[j]] == j.
 * merged_out: NULL, or [n][17][H][W] fp32 (device, overlapping neither input) that the same launch fills with every merged value; when NULL no store is issued.
 * geom, geom_kind, aspect, refine, out_layout, out, coco_scratch, stream: exactly as kasf_heatmap_keypoints takes them.  One launch, plus kasf_coco_h36m's for
 * KASF_LAYOUT_H36M; nothing is allocated.  n = 0 does nothing.  Error 2, before a device or a pointer is touched: every refusal of kasf_heatmap_keypoints, a
 * null hm_flipped with n > 0, a partner that is no involution on 0..16, merged_out equal to hm or hm_flipped. */
int kasf_heatmap_flip_keypoints(const void* hm, const void* hm_flipped, int32_t dtype, int64_t n, int32_t H, int32_t W,
                                const int32_t* partner /* host, 17 entries, NULL = COCO pairs */, int32_t shift,
                                const float* geom, int32_t geom_kind, double aspect, int32_t refine, int32_t out_layout,
                                float* out, float* coco_scratch, float* merged_out /* may be NULL */, void* stream);

/* ---- pose-network heatmaps -> keypoints with DARK / UDP sub-pixel refinement (ADDED under ABI 12: additive, kasf_version() stays 12; look it up by name) ----
 * kasf_heatmap_keypoints (hm_flipped = NULL) or kasf_heatmap_flip_keypoints (hm_flipped given) with the refinement and the affine that ViTPose and the *_dark /
 * *_udp HRNet checkpoints are trained and evaluated with, in the same ONE launch: the quarter-pixel rule is off by up to a quarter of a heatmap pixel by
 * construction, these are not.  The library is built with -ffp-contract=off and every rule below names its precision and order, so a numpy restatement performs
 * the same IEEE operations (tests/test_heatmap_dark_cpu.py) and the device is held to it bit for bit.
 *   mode      KASF_DECODE_QUARTER   kasf_heatmap_keypoints' refine rule (with udp = 0 the call computes what the existing entries compute)
 *             KASF_DECODE_DARK      DARK, Zhang et al., CVPR 2020 "Distribution-Aware Coordinate Representation": mmpose's post_process = 'unbiased'
 *             KASF_DECODE_DARK_UDP  the DARK step of UDP, Huang et al., CVPR 2020 "The Devil is in the Details": mmpose's post_dark_udp, what ViTPose's
 *                                   use_udp = True, modulate_kernel = 11 selects
 *   common    the argmax (py, px) and the score bv come from the RAW map -- from the merged map under hm_flipped, merged exactly as kasf_heatmap_flip_keypoints
 *             merges --, by the total order and the "bv > 0" mask of kasf_heatmap_keypoints; with a false mask the coordinates are 0 and no step is made.  16-bit
 *             inputs are widened exactly; raw(y, x) below is that map's value as fp32.
 *   weights   w[0 .. K - 1], K odd, 1 <= K <= 17: the separable Gaussian, a HOST array read during the call and passed by value into the launch (unread with
 *             KASF_DECODE_QUARTER).  The Python helper gaussian_weights(K, sigma) computes them in fp64 and rounds once to fp32: without sigma and for K = 1, 3, 5, 7
 *             OpenCV's fixed tables [1], [.25, .5, .25], [.0625, .25, .375, .25, .0625], [.03125, .109375, .21875, .28125, .21875, .109375, .03125]; otherwise
 *             sigma = ((K - 1) * 0.5 - 1) * 0.3 + 0.8 when none is given, w_i = exp(-(i - (K - 1) / 2)^2 / (2 sigma^2)), divided by their sum.
 *   blur      blur(y, x), fp32, separable, horizontal first, r = K / 2: h(yy) = sum over kh = 0 .. K - 1, ascending, of w[kh] * raw_b(yy, x + kh - r); blur = sum
 *             over kv = 0 .. K - 1, ascending, of w[kv] * h(y + kv - r); each product rounded, then added, accumulators starting at 0.0f.  raw_b is the border
 *             rule: DARK zero outside the map (mmpose zero-pads by r, so OpenCV's own border never enters); DARK_UDP reflect-101 (-i -> i, n - 1 + i -> n - 1 - i),
 *             repeated with period 2 (n - 1) for maps narrower than the radius, n = 1 always reading index 0.  DARK deliberately omits mmpose's renormalisation
 *             "* origin_max / max(blurred)": a constant factor, hence an additive constant after the logarithm, which cancels in every difference below; it could
 *             matter only through the 1e-10 clamp.
 *   log       L(v), fp64, the library's own routine: frexp gives m in [0.5, 1) and e; if m < 0.7071067811865476 then m = 2 m, e = e - 1; s = (m - 1) / (m + 1),
 *             z = s * s; p by Horner from 1 / 23 down over the odd denominators 21, 19, ... 1, each step p = p * z + 1.0 / d; L = e * 0.6931471805599453 +
 *             2.0 * s * p.  +inf and NaN are returned as they are.  Within 4.4e-16 relative of the correctly rounded logarithm on [1e-10, 50].
 *             clamps: max(v, lo) = v < lo ? lo : v and min(v, hi) = v > hi ? hi : v, so a NaN stays a NaN.
 *   DARK      made only if 1 < px < W - 2 and 1 < py < H - 2.  g(dy, dx) = L(max((double)blur(py + dy, px + dx), 1e-10));
 *             gx = 0.5 * (g(0,1) - g(0,-1)), gy = 0.5 * (g(1,0) - g(-1,0)); a = 0.25 * (g(0,2) - 2 g(0,0) + g(0,-2)), d = 0.25 * (g(2,0) - 2 g(0,0) + g(-2,0)),
 *             b = 0.25 * (g(1,1) - g(-1,1) - g(1,-1) + g(-1,-1)); det = a * d - b * b; if det == 0 there is no step.
 *   DARK_UDP  always made.  g(dy, dx) = L(min(max((double)blur(clamp(py + dy, 0, H - 1), clamp(px + dx, 0, W - 1)), 0.001), 50.0)), the clamp of the position
 *             being mmpose's edge padding of the blurred map; gx, gy as above; a = g(0,1) - 2 g(0,0) + g(0,-1) + eps, d = g(1,0) - 2 g(0,0) + g(-1,0) + eps,
 *             b = 0.5 * (g(1,1) - g(0,1) - g(1,0) + g(0,0) + g(0,0) - g(0,-1) - g(-1,0) + g(-1,-1)), eps = 2^-23; det = a * d - b * b.
 *   step      fp64, left to right as written: x = px - (d * gx - b * gy) / det, y = py - (a * gy - b * gx) / det.  Nothing bounds the step, as in both
 *             published procedures; infinities and NaNs propagate.
 *   to image  udp = 0: kasf_heatmap_keypoints' affine, cx + (x - W / 2) kx and cy + (y - H / 2) ky.  udp != 0 (H, W >= 2): sw = fl32(scale_x * 200),
 *             sh = fl32(scale_y * 200), x_img = fl32((double)cx + (x - (W - 1) * 0.5) * ((double)sw / (W - 1))), y_img likewise with sh, H, cy: heatmap
 *             coordinates over W - 1 / H - 1 intervals, each axis by its own scale.  x, y stay fp64 from the step to this single rounding.  udp with
 *             KASF_DECODE_QUARTER is allowed.  UDP on the crop side is not part of this entry: udp is for crops the caller made the UDP way.
 * hm_flipped, partner, shift, merged_out: as kasf_heatmap_flip_keypoints takes them; hm_flipped = NULL means no flip test, and partner (checked when given), shift
 * are then unused and merged_out must be NULL.  geom, geom_kind, aspect, out_layout, out, coco_scratch, stream: as kasf_heatmap_keypoints takes them.  One launch,
 * plus kasf_coco_h36m's for KASF_LAYOUT_H36M; nothing is allocated.  n = 0 does nothing.  Error 2, before a device or a pointer is touched: every refusal of the two
 * existing entries, a mode out of range, K even or outside 1 .. 17, weights NULL with a mode other than KASF_DECODE_QUARTER, udp with H < 2 or W < 2.
 * NOT VERIFIED: the rules restate mmpose's two procedures and OpenCV's GaussianBlur (its kernel tables, its sigma rule, its reflect-101 border) from their published
 * arithmetic; neither mmpose nor an OpenCV build was available to record a decode from, and cv2's SIMD blur may round differently, so equality with a particular
 * mmpose / cv2 build is not verified and no bit equality with one is claimed. */
#define KASF_DECODE_QUARTER 0
#define KASF_DECODE_DARK 1
#define KASF_DECODE_DARK_UDP 2
int kasf_heatmap_decode(const void* hm, const void* hm_flipped /* NULL: no flip test */, int32_t dtype, int64_t n, int32_t H, int32_t W,
                        const int32_t* partner /* host, 17 entries, NULL = COCO pairs */, int32_t shift,
                        const float* geom, int32_t geom_kind, double aspect, int32_t mode, const float* weights /* host, K floats, read during the call */,
                        int32_t K, int32_t udp, int32_t out_layout, float* out, float* coco_scratch, float* merged_out /* may be NULL */, void* stream);

/* ---- YOLOv3 detector output -> person boxes in frame pixels (ADDED under ABI 12: additive, kasf_version() stays 12; a library without it fails to load on the
 * missing symbol).  Replaces, on the device and without a host synchronisation, what yolo_human_det does behind the detector network (human_detector.py:116-168):
 * predict_transform (util.py:34-81), write_results with det_hm (util.py:107-225) and the un-letterbox (human_detector.py:144-153).  Two launches on `stream`.
 * src [n_src] (a HOST array of DEVICE pointers), of KASF_DTYPE_F32, _F16 or _BF16 (the 16-bit types are widened to fp32 on load, which is exact; every rule is on
 * the fp32 values), contiguous, only read:
 *   KASF_DETECT_PREDICTION  n_src = 1, src[0] = prediction [batch][N][5 + C] with N = grid[0]: what Darknet.forward returns (x, y, w, h at network-input scale,
 *                           objectness, C class scores; already through predict_transform).  A, anchors are ignored.
 *   KASF_DETECT_HEADS       src[k] = raw head [batch][A * (5 + C)][G_k][G_k], G_k = grid[k], as the conv layer in front of each detection layer writes it; anchors
 *                           (HOST) [n_src][A][2] = the (w, h) pixel pairs of head k.  N = sum_k G_k^2 A.
 * RULES.
 *  1 candidate index   its position in the reference's concatenated prediction: heads in the given order, within a head (cy * G + cx) * A + a; in the prediction
 *                      form the row number.
 *  2 box decode        (heads form only) stride = inp_dim / G (inp_dim % G != 0 is refused); x = (sigmoid(tx) + cx) * stride, y likewise; w = exp(tw) *
 *                      fl32(anchor_w / stride) * stride, h likewise; objectness and class score = sigmoid of their logits; all fp32, in this order.  The device's
 *                      exp is not the host's: results sit within a few ulp of the reference's, not on its bits.
 *  3 threshold         a candidate passes when objectness > confidence: strict, fp32.
 *  4 person filter     keep a candidate only if the arg-max of its C class values is class_id; the values are compared with > from class 0 on, so the FIRST maximum
 *                      wins (and a NaN neither wins nor, in first place, loses).  In the heads form the arg-max is taken on the logits and one sigmoid is computed for
 *                      the winner, not C: this differs from the reference only where two class logits round to the same fp32 sigmoid.
 *  5 corners           x1 = x - w / 2, y1 = y - h / 2, x2 = x + w / 2, y2 = y + h / 2, at network-input scale.
 *  6 order             descending objectness; equal objectness: the lower candidate index first (torch.sort leaves that undefined; here it is defined).
 *  7 NMS               greedy in that order at network-input scale; IoU as bbox_iou (bbox.py:51-78): sides (x2 - x1 + 1), intersection sides max(. + 1, 0), iou =
 *                      inter / (a1 + a2 - inter), fp32.  A later box survives a kept one iff iou < nms (an equal IoU, or a NaN one, is suppressed).
 *  8 un-letterbox      fp32: sf = min((1 / width) * inp_dim, (1 / height) * inp_dim) -- two roundings each, as torch evaluates `number / tensor` --; x -= (inp_dim - sf * width) / 2, y -= (inp_dim - sf * height) / 2; both / sf; x clamped
 *                      to [0, width], y to [0, height].  frame_wh (device) [batch][2] = width, height of each image's frame.
 *  9 caps              only the max_candidates best candidates by rule 6 enter NMS (1 <= max_candidates <= KASF_DETECT_MAX_CANDIDATES = 4,096: sort and NMS run in
 *                      the 160 KiB of LDS of one CU), only the first max_boxes survivors are written (1 <= max_boxes <= max_candidates).  Greedy NMS depends only on
 *                      better-ranked boxes, so a capped result is exactly a prefix of the uncapped one.  count[b][1] shows whether the candidate cap bit.
 * 10 differences from the reference, deliberate:  images of a batch are independent (write_results returns at the first image without a person, util.py:156-157;
 *                      here such an image has count 0 and the others are unaffected).  A candidate whose objectness is NaN, or one of whose four corners is not
 *                      finite, is dropped before it is counted (the reference keeps NaN * 0 rows).  The host-side round(i, 2) of human_detector.py:161 and the SORT
 *                      tracker behind it are not part of this.  With confidence < 0 a zero or negative objectness passes and is ordered by its value (the
 *                      reference's nonzero() filter would drop an exact 0).
 * 11 determinism       the same bits from run to run, and an image's result does not depend on what else is in the batch: no atomics; candidates are selected and
 *                      ordered by the key (objectness, index) alone, through an order-preserving map of the fp32 bits.
 * OUTPUT (device).  boxes [batch][max_boxes][6] fp32 = x1, y1, x2, y2 (frame pixels), objectness, class score; index [batch][max_boxes] int32 = candidate index of
 * each row; count [batch][2] int32 = rows written, candidates that passed rules 3, 4 and 10 before any cap.  Rows past the count are 0 (index: -1).
 * workspace (device, 16-byte aligned): kasf_detect_workspace_bytes(batch, N, max_candidates) bytes (28 per candidate slot; negative on a refused shape), contents undefined before
 * and after.  batch = 0 does nothing.  Error 2, before a device or a pointer is touched: a null pointer (src, src[k], grid, frame_wh, boxes, index, count, workspace;
 * anchors in the heads form), batch outside [0, 65535], n_src outside 1..4 (or not 1 in the prediction form), A outside 1..8, C < 1, class_id outside [0, C), a grid
 * outside [1, 4096] or not dividing inp_dim, N outside [1, 2^24], the caps out of range, confidence or nms not finite, an unknown form or dtype, workspace too small or not 16-byte aligned. */
#define KASF_DETECT_PREDICTION 0
#define KASF_DETECT_HEADS 1
#define KASF_DETECT_MAX_CANDIDATES 4096
int64_t kasf_detect_workspace_bytes(int32_t batch, int64_t n_per_image, int32_t max_candidates);
int kasf_detect_boxes(const void* const* src, int32_t n_src, int32_t form, int32_t dtype, int32_t batch, const int32_t* grid, int32_t A, int32_t C,
                      const float* anchors, int32_t inp_dim, const float* frame_wh, float confidence, float nms, int32_t class_id, int32_t max_candidates,
                      int32_t max_boxes, float* boxes, int32_t* index, int32_t* count, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- person boxes -> pose-network inputs (ADDED under ABI 12: additive, kasf_version() stays 12; a library without it fails to load on the missing symbol).
 * Replaces, on the device, the demo's PreProcess (utilitys.py:139-169): per person box_to_center_scale, get_affine_transform, cv2.warpAffine(frame, trans,
 * (out_w, out_h), INTER_LINEAR), ToTensor, Normalize, torch.cat and the [:, [2, 1, 0]] swap of gen_kpts.py:155.  One launch on `stream`; the library allocates nothing.
 * frames: uint8 (device), n_frames images of Hf rows of Wf pixels of 3 interleaved channels; pixel (f, y, x) channel c is the byte at
 * frames + f * frame_stride + y * row_stride + 3 * x + c.  row_stride >= 3 * Wf: a decoder's padded pitch is read in place.  frames is only read.
 * frame_index [n] int32 (device): the frame each person is cropped from; may be NULL when n_frames == 1 (every person from frame 0).  A value outside
 * [0, n_frames) cannot be refused without a synchronisation: that person comes out as an all-border crop (rule 3 with every tap outside).
 * geom [n][4] fp32 (device), geom_kind, aspect: exactly as kasf_heatmap_keypoints takes them.
 * out [n][3][out_h][out_w] (device) of out_dtype = KASF_DTYPE_F32, _F16 or _BF16.  mean_std: a HOST pointer to six floats, mean[0..2] then std[0..2], indexed by the
 * FRAME's channel (rule 4), read during the call and passed by value into the launch.  center_scale_out [n][4] fp32 (device; may be NULL).
 * RULES.
 *  1 geometry    center (cx, cy) and scale (scale_x, scale_y) as fp32: given, or derived from the box as kasf_heatmap_keypoints derives them, with
 *                scale_y = fl32(box height grown to the aspect / 200) (* 1.25 in fp32 unless cx == -1).  The map from crop pixel (x, y) to frame position is the
 *                closed form of get_affine_transform(center, scale, 0, (out_w, out_h), inv = 1), the one kasf_heatmap_keypoints applies, with out_w, out_h in
 *                place of the heatmap's W, H: anchors sw = fl32(scale_x * 200), s1y = fl32(cy - sw / 2), dy = fl32(cy - s1y), s2x = fl32(cx - dy); then in fp64
 *                kx = (cx - s2x) / (out_w / 2), ky = (cy - s1y) / (out_w / 2) (both by out_w / 2; only scale_x enters, as in the reference),
 *                bx = cx - (out_w / 2) kx, by = cy - (out_h / 2) ky.  Position of (x, y): (bx + kx x, by + ky y).
 *  2 positions   on a 1/32-pixel grid, by the 10-bit fixed-point scheme of OpenCV's portable warpAffine; rint = round half to even, integers are 64-bit (where
 *                they fit 32 bits they are the same numbers; a rounded value beyond +-2^61 saturates there).  Column x: ad[x] = rint((kx x) 1024).  Row y:
 *                X0 = rint(bx 1024) + 16, Y0 = rint((ky y + by) 1024) + 16.  X = (X0 + ad[x]) >> 5, Y = Y0 >> 5 (arithmetic shifts).  The tap is (X >> 5, Y >> 5),
 *                the fractions are fx = X & 31, fy = Y & 31.  If any of kx, ky, bx, by is not finite the whole crop is border.
 *  3 value       per channel, with p00 the tap, p01 its right, p10 its lower and p11 its lower right neighbour, each counted 0 on its own when it lies outside
 *                the frame (BORDER_CONSTANT 0): S = (32 - fx)(32 - fy) p00 + fx (32 - fy) p01 + (32 - fx) fy p10 + fx fy p11, v = (S + 512) >> 10, an integer
 *                0..255.  This is the 15-bit-weight form (32 S + 16384) >> 15, the weights being exact multiples of 32.  No antialiasing when the box is larger
 *                than the crop (the reference has none either).
 *  4 normalise   f = ((float)v / 255.0f - mean[c]) / std[c] in fp32, every operation rounded once, c the FRAME's channel.  With swap_rb != 0 output plane k holds
 *                frame channel 2 - k, otherwise channel k.  This reproduces the demo as it is: it normalises the BGR frame with the RGB constants by position and
 *                swaps afterwards, so the red plane is normalised with 0.406 / 0.225.  fp16 / bf16 outputs are the round-to-nearest-even of that fp32 value.
 *  5 outputs     center_scale_out [p] = cx, cy, scale_x, scale_y of rule 1: what kasf_heatmap_keypoints takes as KASF_GEOM_CENTER_SCALE for the heatmaps of this crop.
 *  6 determinism no atomics; a person's result depends on its geom row and its frame alone, not on n or its place in the batch; the same bits from run to run.
 * NOT VERIFIED: rules 2 and 3 restate OpenCV's portable (non-SIMD) warpAffine / remap from its documented arithmetic; no OpenCV build was available to
 * record a crop from, so equality with a particular cv2 build is unverified.  Rule 1 stands in for cv2.getAffineTransform's solve and cv2.warpAffine's own inversion of the
 * forward matrix; against the fp64 inverse of the reference's forward matrix kx, ky, bx, by agree to 1e-12 relative (tests/test_crop_cpu.py).
 * n = 0 does nothing.  Error 2, before a device or a device pointer is touched: n < 0; out_w or out_h outside 1..32767; Hf or Wf outside 1..32767; n_frames < 1;
 * row_stride < 3 * Wf; a negative frame_stride with n_frames > 1; an unknown out_dtype or geom_kind; aspect <= 0 (or NaN) with KASF_GEOM_BOX; mean_std null, or a std that is 0
 * or not finite; with n > 0 a null frames, geom or out, or a null frame_index with n_frames > 1. */
int kasf_crop_persons(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride, const int32_t* frame_index,
                      const float* geom, int32_t geom_kind, double aspect, int64_t n, void* out, int32_t out_dtype, int32_t out_w, int32_t out_h,
                      const float* mean_std, int32_t swap_rb, float* center_scale_out, void* stream);

/* ---- video frames -> detector inputs (ADDED under ABI 12: additive, kasf_version() stays 12; a caller checks for the two symbols by name).
 * Replaces, on the device, the demo's prep_image (demo/lib/yolov3/preprocess.py:9-38, called at human_detector.py:131): letterbox_image = cv2.resize(frame,
 * (new_w, new_h), INTER_CUBIC) placed on a canvas of 128, the [:, :, ::-1] channel reversal, the transpose to planes and float().div(255.0).  One launch on
 * `stream` that writes EVERY element of out, padding included (no memset in front of it); the library allocates nothing.
 * frames: uint8 (device), n_frames images of Hf rows of Wf pixels of 3 interleaved channels, all of one Hf x Wf; pixel (f, y, x) channel c is the byte at
 * frames + f * frame_stride + y * row_stride + 3 * x + c, exactly as kasf_crop_persons reads it.  row_stride >= 3 * Wf: a decoder's padded pitch is read in
 * place.  frames is only read.  out [n_frames][3][out_h][out_w] (device) of out_dtype = KASF_DTYPE_F32, _F16 or _BF16.  out_w and out_h are at most
 * KASF_LETTERBOX_MAX_SIDE = 4096: the kernel keeps one table entry per output column in LDS (12 bytes each, 48 KiB at the limit).
 * RULES.
 *  1 geometry    letterbox_image in C doubles (the IEEE operations of the reference's Python floats): r = min((double)out_w / Wf, (double)out_h / Hf);
 *                new_w = (int)(Wf * r), new_h = (int)(Hf * r), by truncation; pad_x = (out_w - new_w) / 2, pad_y = (out_h - new_h) / 2, by integer division.
 *                The resized image occupies rows [pad_y, pad_y + new_h) and columns [pad_x, pad_x + new_w) of every plane; everything else is padding.
 *                kasf_letterbox_plan returns these four numbers (host only, no device); new_w < 1 or new_h < 1 -- a frame so elongated that the reference's
 *                cv2.resize would raise -- is error 2.
 *  2 positions   per axis, shown for x (y: Hf, new_h, dy): scale_x = 1.0 / ((double)new_w / (double)Wf), two roundings in that order;
 *                fx = (float)((dx + 0.5) * scale_x - 0.5) for column dx of the resized image, product and subtraction in double and not contracted;
 *                sx = floorf(fx), t = fx - sx in fp32.  The four weights in fp32 with A = -0.75f, every operation rounded once, in exactly this order:
 *                  c0 = ((A*(t+1) - 5*A)*(t+1) + 8*A)*(t+1) - 4*A       c1 = ((A+2)*t - (A+3))*t*t + 1
 *                  c2 = ((A+2)*(1-t) - (A+3))*(1-t)*(1-t) + 1           c3 = 1 - c0 - c1 - c2   (left to right)
 *                a[k] = (int)rintf(c[k] * 2048.0f), round half to even; every value fits a short.  b[k] is the same for a row.
 *  3 value       integers only.  Tap k of an axis is source index clamp(sx - 1 + k, 0, Wf - 1): the edge is replicated; rows clamp the same way with Hf.
 *                V = sum_ky b[ky] * sum_kx a[kx] * src[row_ky][col_kx][c];  v = clamp((V + (1 << 21)) >> 22, 0, 255), an arithmetic shift.  |V| < 2^31 for every
 *                frame (255 * 1.375^2 * 2^22 = 2.02e9 bounds it; 1.53e9 is the largest seen, on frames of 0 / 255 noise), and integer sums are exact, so the
 *                16-tap form and a horizontal-then-vertical form give the same v.  No antialiasing when shrinking (the reference has none either).
 *  4 output      plane k of a resized pixel is (float)v / 255.0f, one fp32 division, of frame channel 2 - k with swap_rb != 0 (the reference's [:, :, ::-1]),
 *                of channel k otherwise.  Padding is (float)pad_value / 255.0f in every plane (the reference: 128).  fp16 / bf16 outputs are the
 *                round-to-nearest-even of that fp32 value.
 *  5 determinism no atomics, no scratch, nothing that depends on n_frames: a frame's planes are a function of that frame alone; the same bits from run to run.
 * ACCURACY of rules 2-3 against exact cubic convolution (fp64, A = -0.75, positions (dx + 0.5) Wf / new_w - 0.5, replicated edge, clamped to [0, 255]):
 * at most 1.25 grey levels on every pixel = 0.5 for the final rounding + about 0.69 for the 11-bit coefficients (each is off by at most 2^-12, so a pass is
 * off by at most 255 * 2^-12 * 4 = 0.25 times the other pass's sum of |weights| <= 1.375: 0.34 for the columns as the rows amplify them, 0.34 for the rows
 * applied to column sums of up to 255 * 1.375) + about 0.03 for the fp32 position at coordinates up to 1920.  Measured worst case: 0.75 (tests/test_letterbox_cpu.py).
 * NOT VERIFIED: rules 2 and 3 restate the fixed-point scheme of OpenCV's portable 8-bit resize(INTER_CUBIC) -- 11-bit coefficients, two passes, a 22-bit
 * rounding shift -- from its documented arithmetic; no OpenCV build was available to record an image from, and cv2's SIMD paths may round differently, so
 * equality with a particular cv2 build is not verified.  The un-letterbox of kasf_detect_boxes keeps the reference's own fp32 offsets, which differ from
 * rule 1's truncated integers by under a pixel, exactly as in the reference.
 * kasf_letterbox_plan: error 2 on Wf or Hf outside 1..32767, out_w or out_h outside 1..4096, a null pointer, or new_w < 1 or new_h < 1.
 * kasf_letterbox_frames: n_frames = 0 does nothing.  Error 2, before a device or a device pointer is touched: n_frames < 0; Hf or Wf outside 1..32767; out_w or
 * out_h outside 1..4096; row_stride < 3 * Wf; frame_stride < 0; frame_stride < Hf * row_stride with n_frames > 1; an unknown out_dtype; pad_value outside
 * 0..255; a plan that fails; with n_frames > 0 a null frames or out. */
#define KASF_LETTERBOX_MAX_SIDE 4096
int kasf_letterbox_plan(int32_t Wf, int32_t Hf, int32_t out_w, int32_t out_h, int32_t* new_w, int32_t* new_h, int32_t* pad_x, int32_t* pad_y);
int kasf_letterbox_frames(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride, void* out, int32_t out_dtype,
                          int32_t out_w, int32_t out_h, int32_t pad_value, int32_t swap_rb, void* stream);

/* ---- decoder surfaces -> BGR frames (ADDED under ABI 12: additive, kasf_version() stays 12; a caller checks for the symbol by name).
 * Replaces, on the device, the YUV 4:2:0 -> BGR conversion that stands behind the demo's cap.read() (demo/lib/hrnet/gen_kpts.py:106,118): a hardware decoder
 * (VCN through rocDecode or VA-API) leaves NV12 surfaces in device memory, a software decoder (FFmpeg yuv420p) planar I420.  The result is the uint8
 * [Hf][Wf][3] frame that kasf_letterbox_frames and kasf_crop_persons read.  One launch on `stream`; the library allocates nothing; the planes are only read.
 * RULES.
 *  1 layouts     8-bit 4:2:0: a luma plane of Hf rows of Wf samples and chroma planes of ch = (Hf + 1) / 2 rows of cw = (Wf + 1) / 2 samples.  Odd Wf / Hf are
 *                legal: the last column / row shares the last chroma sample.  Luma sample (f, y, x) is the byte at y + f * y_frame_stride + y * y_row_stride + x.
 *                KASF_YUV_NV12: c0 is ONE interleaved plane, chroma sample (cy, cx) is the byte pair U, V at c0 + f * c_frame_stride + cy * c_row_stride + 2 * cx;
 *                c1 must be NULL.  KASF_YUV_I420: c0 is the U plane and c1 the V plane, one byte per sample at + f * c_frame_stride + cy * c_row_stride + cx
 *                (both planes share the two strides).  Strides are in bytes; no alignment is asked of any pointer or stride.
 *  2 siting      nearest: pixel (y, x) takes chroma sample (y >> 1, x >> 1), as cv2.cvtColor(COLOR_YUV2BGR_NV12 / _I420) does.  Interpolated chroma
 *                (bilinear upsampling, co-sited or centred) is out of scope.
 *  3 arithmetic  integers only, 20 fractional bits.  y1 = max(0, Y - 16) * CY with full_range == 0, Y * CY otherwise; u = U - 128, v = V - 128;
 *                  R = sat8((y1 + CVR * v + (1 << 19)) >> 20)
 *                  G = sat8((y1 + CVG * v + CUG * u + (1 << 19)) >> 20)
 *                  B = sat8((y1 + CUB * u + (1 << 19)) >> 20)
 *                the shift is arithmetic and sat8 clamps to 0..255.  Every intermediate fits int32: y1 <= 255 * 1220945 < 3.12e8, |u|, |v| <= 128 and the largest
 *                chroma term is 128 * 2215014 < 2.84e8 (G: 128 * (852492 + 409993) < 1.62e8), so |sum| < 3.12e8 + 2.84e8 + 2^19 < 5.97e8 < 2^31; integer sums are
 *                exact, so any grouping of the terms gives the same bits.
 *  4 tables      { CY, CVR, CVG, CUG, CUB } per (matrix, range), the literals below.  KASF_YUV_BT601 limited is OpenCV's five published constants =
 *                rint(c * 2^20) of 1.164, 1.596, 0.813, 0.391, 2.018.  The other three are rint(c * 2^20) of the exact doubles from Kr, Kb (0.299 / 0.114 for
 *                BT.601, 0.2126 / 0.0722 for BT.709), Kg = 1 - Kr - Kb, the luma scale ls (255 / 219 limited, 1 full) and the chroma scale cs (255 / 224
 *                limited, 1 full): CY = ls, CVR = 2 (1 - Kr) cs, CVG = -2 (1 - Kr) Kr / Kg cs, CUG = -2 (1 - Kb) Kb / Kg cs, CUB = 2 (1 - Kb) cs.
 *  5 output      out[f][y][x][0..2] = B, G, R, or R, G, B with rgb != 0, uint8, at out + f * out_frame_stride + y * out_row_stride + 3 * x.  out_row_stride >=
 *                3 * Wf: a caller's pitched buffer is written in place.  Every byte of the 3 * Wf payload of every row is written; no byte of the row padding is.
 *  6 determinism no atomics, no scratch, no LDS: a pixel is a function of its three samples alone; the same bits from run to run and for a frame alone or in a batch.
 * ACCURACY of rules 3-4 against the exact fp64 conversion (the same Kr, Kb and scales, the same max(0, Y - 16), clamped to [0, 255]), over all 2^24 (Y, U, V): at
 * most 0.5 + sum |c_int / 2^20 - c_exact| * max|operand| grey levels per channel (operands: 239 or 255 for luma, 128 for chroma) = about 0.8 for BT.601
 * limited, whose constants are three-decimal roundings, and under 0.5003 for the derived tables (tests/test_yuv_cpu.py).
 * NOT VERIFIED: rules 2 and 3 restate the fixed-point scheme of OpenCV's portable cvtColor for 4:2:0 input from its documented arithmetic; what
 * cv2.VideoCapture.read() returns additionally depends on the FFmpeg build behind it.  No OpenCV build was available to record a frame from, so equality
 * with a particular cv2 / FFmpeg build is not verified.
 * n_frames = 0 does nothing.  Error 2, before a device or a device pointer is touched: n_frames < 0; Hf or Wf outside 1..32767; y_row_stride < Wf;
 * c_row_stride < 2 * cw (NV12) or < cw (I420); out_row_stride < 3 * Wf; a negative frame stride; with n_frames > 1 y_frame_stride < Hf * y_row_stride,
 * c_frame_stride < ch * c_row_stride or out_frame_stride < Hf * out_row_stride; an unknown layout or matrix; a non-null c1 with NV12 or a null c1 with
 * I420; with n_frames > 0 a null y, c0 or out. */
#define KASF_YUV_NV12 0
#define KASF_YUV_I420 1
#define KASF_YUV_BT601 0
#define KASF_YUV_BT709 1
#define KASF_YUV_COEF_BT601_LIMITED { 1220542, 1673527, -852492, -409993, 2116026 }
#define KASF_YUV_COEF_BT601_FULL    { 1048576, 1470104, -748826, -360853, 1858077 }
#define KASF_YUV_COEF_BT709_LIMITED { 1220945, 1879825, -558796, -223607, 2215014 }
#define KASF_YUV_COEF_BT709_FULL    { 1048576, 1651297, -490864, -196424, 1945738 }
int kasf_yuv420_to_bgr(const void* y, const void* c0, const void* c1, int32_t layout, int32_t n_frames, int32_t Hf, int32_t Wf,
                       int64_t y_row_stride, int64_t c_row_stride, int64_t y_frame_stride, int64_t c_frame_stride,
                       void* out, int64_t out_row_stride, int64_t out_frame_stride,
                       int32_t matrix, int32_t full_range, int32_t rgb, void* stream);

/* ---- skeletons over the frame, and the encoder's NV12 surface (ADDED under ABI 12: additive, kasf_version() stays 12; a caller checks for the symbols by name).
 * Replaces, on the device, the demo's plot_on_frame (demo/demo.py:91-105: cv2.line and cv2.circle per bone on a copy of the frame), the score threshold of
 * plot_keypoint / write (demo/lib/hrnet/lib/utils/utilitys.py:24-58) and the host frame that cv2.VideoWriter takes (demo/demo.py:307-323).  kasf_draw_poses
 * paints the tracked skeletons and filled rectangles over the uint8 frame and writes the painted frame, its NV12 surface, or both, as ONE launch on `stream`;
 * kasf_bgr_to_nv12 is the same launch with nothing to paint: the inverse of kasf_yuv420_to_bgr.  The library allocates nothing; the inputs are only read.
 *   frames    uint8 [n_frames][Hf][Wf][3] = B, G, R (R, G, B with rgb != 0): pixel (f, y, x) at frames + f * frame_stride + y * row_stride + 3 * x (bytes),
 *             what kasf_yuv420_to_bgr writes and kasf_crop_persons reads.
 *   keypoints fp32 [n_frames][P][J][C], C = 2 (x, y) or 3 (x, y, score) in frame pixels: element (f, p, j, c) at keypoints + f * kp_frame_stride +
 *             p * kp_person_stride + j * kp_joint_stride + c * kp_coord_stride (ELEMENTS).  1 <= J <= 32.  valid uint8 [n_frames][P] behind two byte strides,
 *             or NULL for every row.
 *   segments  int32 [S][2] joint pairs, colors uint8 [S][3] in the frame's channel order (device memory), 0 <= S <= 32; a pair that names a joint outside
 *             0..J-1 makes that joint not visible.  dot_color[3]: HOST memory, read before the call returns.  thickness t in 1..64, dot_radius r in 0..32.
 *   fills     int32 [R][7] = x0, y0, x1, y1, c0, c1, c2 (device memory, the same for every frame), R <= 8: the half-open rectangle [x0, x1) x [y0, y1) clipped
 *             to the frame, painted with the low 8 bits of c0, c1, c2.
 *   out_bgr   as frames, behind its own strides; it may be exactly `frames` with the same strides (in place) or disjoint from it -- any other overlap is the
 *             caller's error and is not detected.  out_y / out_uv: an NV12 surface, luma (f, y, x) at out_y + f * y_frame_stride + y * y_row_stride + x, the
 *             pair U, V of chroma sample (cy, cx) at out_uv + f * uv_frame_stride + cy * uv_row_stride + 2 * cx.  out_bgr may be NULL, or out_y and out_uv
 *             both, not all three.  Strides are in bytes; no alignment is asked of any pointer or stride.
 * RULES.  All geometry is in integers and exact.
 *  1 joints      xi = trunc(x), yi = trunc(y), toward zero (Python's int() in plot_on_frame: int(-0.5) = 0).  Joint (f, p, j) is VISIBLE iff x and y are finite,
 *                -32768 <= xi, yi <= 65535, valid is NULL or valid[f][p] != 0, and -- with C = 3 and a finite min_score -- score > min_score (a NaN score is not
 *                visible; a NaN or infinite min_score switches the test off).  Pixels are 0 <= px, py <= 32766.  So with d = B - A and w = pixel - A every
 *                component has |.| <= 98303 < 2^17, and L2 = d . d, s = w . d, w . w and c = w x d are below 2^35 in magnitude.
 *  2 order       painting is opaque: fills 0..R-1, then persons p = 0..P-1 and within a person for s = 0..S-1 line s, the dot at its first joint, the dot at
 *                its second joint (plot_on_frame's loop).  A line is drawn iff both its joints are visible, a dot iff its joint is.  The output pixel is the
 *                colour of the LAST primitive in this order that covers it, else the input pixel.
 *  3 coverage    a dot at A covers (px, py) iff wx^2 + wy^2 <= r^2 (r = 0: the one pixel).  Line A -> B covers it iff the squared distance from the pixel to
 *                the closed segment is <= (t / 2)^2: if L2 = 0 or s <= 0, iff 4 (w . w) <= t^2; if s >= L2, the same with u = w - d; otherwise iff
 *                4 c^2 <= t^2 L2.  4 (w . w) < 2^38 and t^2 L2 <= 2^12 * 2^35 = 2^47 fit int64; 4 c^2 alone could reach 2^72, but |d| <= |dx| + |dy|, so
 *                2 |c| > t (|dx| + |dy|) implies 4 c^2 > t^2 L2: not covered, decided with operands below 2^37; otherwise 2 |c| <= 64 * 196606 < 2^24 and
 *                4 c^2 < 2^48.  Every intermediate fits int64.
 *  4 NOT cv2     this is exact Euclidean geometry.  It is NOT a restatement of OpenCV's polygon-fill ThickLine or of its midpoint circle, whose pixels differ
 *                at the rim; NOT VERIFIED against any cv2 build, and no equality with cv2.line / cv2.circle is claimed.  Anti-aliasing, alpha, text: out of scope.
 *  5 surface     from the PAINTED pixels.  Y = sat8((CRY R + CGY G + CBY B + (yoff << 20) + (1 << 19)) >> 20), yoff = 16 (limited) or 0 (full).  One chroma
 *                sample per 2 x 2 quad from the sums S_R, S_G, S_B of its four painted pixels -- at an odd right / bottom edge the last column / row is
 *                replicated, so there are always four --: U = sat8((CRU S_R + CGU S_G + CH S_B + (128 << 22) + (1 << 21)) >> 22),
 *                V = sat8((CH S_R + CGV S_G + CBV S_B + (128 << 22) + (1 << 21)) >> 22); shifts are arithmetic.  The literals below are
 *                { CRY, CGY, CBY, CRU, CGU, CH, CGV, CBV } = rint(c * 2^20) of the exact doubles from Kr, Kb (0.299 / 0.114, 0.2126 / 0.0722), Kg = 1 - Kr - Kb,
 *                ls = 219 / 255 and cs = 224 / 255 (limited) or 1 (full): Kr ls, Kg ls, Kb ls, -Kr cs / (2 (1 - Kb)), -Kg cs / (2 (1 - Kb)), cs / 2 (= CBU = CRV:
 *                eight distinct coefficients), -Kg cs / (2 (1 - Kr)), -Kb cs / (2 (1 - Kr)) -- the same four (matrix, range) pairs as KASF_YUV_COEF_*.
 *                int32: luma <= 255 * 2^20 + 2^24 + 2^19 < 2.9e8; chroma sums are <= 1020 and |CRU| + |CGU| = |CGV| + |CBV| = CH <= 524288, so each sum lies
 *                in [-5.35e8, 5.35e8] + 5.37e8 + 2^21, inside (-2^31, 2^31).
 *  6 determinism no atomics and no scratch; a pixel is a function of the frame's primitives and its own quad: the same bits from run to run, for a frame alone
 *                or in a batch, whatever the tiling.  Every byte of the 3 * Wf payload of out_bgr's rows is written (in place, a byte that no primitive covers
 *                keeps its value), every byte of the Wf luma payload and of the 2 * ((Wf + 1) / 2) chroma payload of the surface's rows; no padding byte is.
 * ACCURACY of rule 5 against the exact fp64 conversion of the pixel (luma) or of the quad's mean (chroma), clamped to [0, 255]: at most
 * 0.5 + sum |c_int / 2^20 - c| * 255 grey levels per channel, under 0.5004 for every table (tests/test_draw_cpu.py).  NOT VERIFIED: what a particular encoder
 * makes of the surface (its matrix and range flags, its chroma siting) is the caller's to set; no equality with an encoder's or cv2's colour handling is claimed.
 * n_frames = 0 does nothing.  Error 2, before a device or a device pointer is touched: n_frames < 0; Hf or Wf outside 1..32767; row_stride or out_row_stride
 * < 3 * Wf; y_row_stride < Wf; uv_row_stride < 2 * ((Wf + 1) / 2); a negative frame stride; with n_frames > 1 a frame stride that does not cover its plane
 * (rows * row stride); all outputs NULL, or one of out_y / out_uv without the other; P < 0 or > 2^20; S outside 0..32; with P > 0 and S > 0: J outside 1..32,
 * C not 2 or 3, a null keypoints, segments or colors; a null dot_color; thickness outside 1..64; dot_radius outside 0..32; R outside 0..8 or R > 0 with a null
 * fills; an unknown matrix; with n_frames > 0 a null frames. */
#define KASF_RGB2YUV_COEF_BT601_LIMITED { 269262, 528618, 102662, -155423, -305128, 460551, -385654, -74897 }
#define KASF_RGB2YUV_COEF_BT601_FULL    { 313524, 615514, 119538, -176932, -347356, 524288, -439026, -85262 }
#define KASF_RGB2YUV_COEF_BT709_LIMITED { 191455, 644067, 65019, -105533, -355018, 460551, -418321, -42230 }
#define KASF_RGB2YUV_COEF_BT709_FULL    { 222927, 749942, 75707, -120138, -404150, 524288, -476214, -48074 }
int kasf_draw_poses(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride,
                    const float* keypoints, int32_t P, int32_t J, int32_t C,
                    int64_t kp_frame_stride, int64_t kp_person_stride, int64_t kp_joint_stride, int64_t kp_coord_stride,
                    const uint8_t* valid, int64_t valid_frame_stride, int64_t valid_person_stride,
                    const int32_t* segments, const uint8_t* colors, int32_t S, const uint8_t* dot_color,
                    int32_t thickness, int32_t dot_radius, float min_score, const int32_t* fills, int32_t R,
                    void* out_bgr, int64_t out_row_stride, int64_t out_frame_stride,
                    void* out_y, void* out_uv, int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride, int64_t uv_frame_stride,
                    int32_t matrix, int32_t full_range, int32_t rgb, void* stream);
int kasf_bgr_to_nv12(const void* frames, int32_t n_frames, int32_t Hf, int32_t Wf, int64_t row_stride, int64_t frame_stride,
                     void* out_y, void* out_uv, int64_t y_row_stride, int64_t uv_row_stride, int64_t y_frame_stride, int64_t uv_frame_stride,
                     int32_t matrix, int32_t full_range, int32_t rgb, void* stream);

/* kasf_pose_panel: the 3-D plot beside the frame (demo/demo.py:159-191), as the projection that puts world-space poses into a panel rectangle for
 * kasf_draw_poses to draw after a background fill.  poses [n][17][3] fp32 (kasf_pose_world's output) -> out [n][17][2] fp32 pixel coordinates; one launch.
 * view = eight HOST floats { ax0, ax1, ax2, ay0, ay1, ay2, cx, cy }, read before the call returns.  For the orthographic view of view_init(elev, azim) into the
 * panel [x0, x1) x [y0, y1) the caller forms them in fp64 and rounds once: right = (-sin az, cos az, 0), up = (-sin el cos az, -sin el sin az, cos el),
 * scale = min(x1 - x0, y1 - y0) / 2 / radius (the demo's RADIUS is 0.72), ax = scale * right, ay = -scale * up (image rows grow downwards),
 * cx = (x0 + x1) / 2, cy = (y0 + y1) / 2.  Per joint, in single fp32 operations in this order, none contracted: d = v - root (joint 0 of the same pose);
 * out_x = (((ax0 * dx) + (ax1 * dy)) + (ax2 * dz)) + cx, out_y likewise with ay and cy.  matplotlib's perspective camera, its axes, ticks and panes are out of
 * scope.  n = 0 does nothing.  Error 2, before a device or a device pointer is touched: n < 0 or n > 2^40; a null view or a view that is not finite; with
 * n > 0 a null poses or out. */
int kasf_pose_panel(const float* poses, int64_t n, const float* view, float* out, void* stream);

/* ---- person boxes -> tracked person boxes (ABI 12): the SORT tracker of demo/lib/sort/sort.py, one launch per tick, no host synchronisation ----
 * state: kasf_sort_state_bytes(streams, slots, max_dets) bytes on the device, 8-byte aligned; ALL ZERO IS AN EMPTY TRACKER, so creating and resetting it (or one
 * stream's part: the bytes divide evenly by streams) is a memset.  Per stream: int32 [16] header (tracks, next id, ticks, held detections, 0 ...), then per list
 * position p < slots x fp64 [7][slots], P fp64 [13][slots] (blocks k < 3 = (cx,vx), (cy,vy), (s,vs): 4k = pos-pos, 4k+1 = pos-vel, 4k+2 = vel-pos, 4k+3 = vel-vel;
 * 12 = r-r), int32 [6][slots] = id, slot, time_since_update, hits, hit_streak, age, then the held detections fp32 [max_dets][4].
 * dets [streams][det_rows][>= 4] fp32 (device; det_rows <= max_dets, the capacity the state was sized for) = x1, y1, x2, y2 in the first four columns, element strides det_stream_stride and det_row_stride (>= 4; columns are
 * adjacent): kasf_detect_boxes' boxes [B][max_boxes][6] as they are.  det_count [streams] int32 (device; NULL = every row): rows that count, clamped to
 * [0, det_rows].  Outputs (device), rows newest track first as Sort.update returns them: boxes [streams][slots][4] fp32 (what kasf_crop_persons takes as
 * KASF_GEOM_BOX), ids (the track's id + 1), slot, born [streams][slots] int32, count, dropped, person_count [streams] int32, persons [streams][num_person][4] fp32.
 * Rows past count are 0 with id -1; rows of persons past person_count are 0.
 *
 * EACH TRACK (sort.py:61-122).  x[7] = (cx, cy, s = w h, r = w / h, vx, vy, vs) and P[7][7], fp64.  F = I with F[0][4] = F[1][5] = F[2][6] = 1, H = the first four
 * rows of I, R = diag(1, 1, 10, 10), P0 = diag(10, 10, 10, 10, 1e4, 1e4, 1e4), Q = diag(1, 1, 1, 1, 0.01, 0.01, 0.01 * 0.01) (sort.py:72-85).
 *  predict     if x[6] + x[2] <= 0 then x[6] *= 0; x = F x; P = F P F^T + Q; age += 1; if time_since_update > 0 then hit_streak = 0; time_since_update += 1.
 *  update      z = (x1 + w / 2, y1 + h / 2, w h, w / h) with w = x2 - x1, h = y2 - y1 of the detection widened to fp64; then y = z - H x, S = H P H^T + R,
 *              K = P H^T S^-1, x = x + K y, P = (I - K H) P (I - K H)^T + K R K^T; time_since_update = 0, hits += 1, hit_streak += 1.  filterpy is not
 *              installed where this was written: the update is RESTATED from the published form of filterpy's KalmanFilter.update, not recorded from it.
 *  box         w = sqrt(x[2] x[3]), h = x[2] / w, corners cx -+ w / 2, cy -+ h / 2.
 * With this F and H and a diagonal P0, P keeps the blocks (cx,vx), (cy,vy), (s,vs) and the scalar r: every other entry is an exact 0 (tests/test_track_cpu.py
 * holds the dense form to that on every test sequence), S is diagonal and S^-1 is four reciprocals.  The kernel carries the 13 numbers of the blocks and leaves out
 * the products with the exact zeros and ones of F and H, which change no finite value; what remains is the dense form's sequence, with contraction off.
 *
 * EACH TICK, per stream, in the reference's order (sort.py:177-222):
 *  1 ticks += 1; predict every track.
 *  2 IoU of every detection (bb_test) against every predicted box (bb_gt) as sort.py:16-30 in fp64, stored rounded to fp32.
 *  3 the assignment of min(detections, tracks) pairs that maximises the sum of those fp32 values (scipy.optimize.linear_sum_assignment of the negated matrix).
 *  4 a pair whose fp32 IoU is below (float)iou_threshold is unmatched again.
 *  5 matched tracks update with their detection.
 *  6 unmatched detections found tracks, appended to the list: first those outside the assignment by ascending index, then those unmatched by rule 4 by
 *    ascending index (scipy returns its rows sorted).  A new track takes the stream's next id and the smallest slot in [0, slots) that no track of the list holds;
 *    it keeps that slot until it dies.  born = 1 on this tick.
 *  7 the list is walked newest first: a track is emitted iff time_since_update < 1 and (hit_streak >= min_hits or ticks <= min_hits), with its box from the
 *    updated state; then it is removed iff time_since_update > max_age.  The list keeps its order.
 * From gen_video_kpts (gen_kpts.py:125-143): with hold_last != 0 a tick without a valid detection runs on the stream's last non-empty set of valid detections
 * (bboxs_pre; none yet: on none); persons[k] = the k-th OLDEST emitted track, k < person_count = min(count, num_person): people_track[-num_person:][::-1].  The
 * host-side round(i, 2) is not applied.
 *
 * DELIBERATELY UNLIKE THE REFERENCE.
 *  - The id counter is per stream; the reference's is one class attribute shared by every Sort object of the process.
 *  - A track whose predicted box has a non-finite coordinate is dropped in step 1.  The reference masks inf rows out of the matrix but pops only NaN ones, after
 *    which its matrix columns no longer line up with its list.
 *  - A detection with a non-finite coordinate or h <= 0 is ignored (it is not part of "the detections" above).  An IoU that is not finite counts as 0.
 *  - Where two assignments have exactly equal sums the choice is this kernel's (shortest augmenting paths, rows = the smaller side in ascending order, among
 *    equal path costs an unassigned column first, then the lower index), which need not be scipy's; scipy promises none.
 *  - When the list is full (slots tracks), further births of step 6 are dropped in that order, take no id, and are counted in dropped.
 *
 * streams = 0 does nothing.  Error 2, before a device or a device pointer is touched: streams outside 0..65535; slots or max_dets outside 1..64 (a track and a
 * detection each take one lane of a wavefront); det_rows outside 0..max_dets; det_row_stride < 4; det_stream_stride < 0; max_age or min_hits < 0; iou_threshold not finite; num_person outside
 * 1..65535; with streams > 0 a null pointer other than det_count (and dets when det_rows = 0), or a state that is not 8-byte aligned.  kasf_sort_state_bytes returns -2 for the first three. */
#define KASF_SORT_MAX 64
int64_t kasf_sort_state_bytes(int32_t streams, int32_t slots, int32_t max_dets);
int kasf_sort_update(void* state, int32_t streams, int32_t slots, int32_t max_dets, const float* dets, int32_t det_rows, int64_t det_stream_stride, int64_t det_row_stride,
                     const int32_t* det_count, int32_t max_age, int32_t min_hits, float iou_threshold, int32_t num_person, int32_t hold_last, float* boxes,
                     int32_t* ids, int32_t* slot, int32_t* born, int32_t* count, int32_t* dropped, float* persons, int32_t* person_count, void* stream);

/* ---- the stream lifter's slots driven by the tracker's output (ADDED under ABI 12: additive, kasf_version stays 12; look the two symbols up by name) ----
 * What a caller of kasf_stream_push / kasf_stream_windows / kasf_stream_emit had to do on the host between kasf_sort_update and the lift -- read ids, slot and
 * count back, decide births and deaths, upload slot ids -- done on the device: two launches per tick, one in front of the model's forward and one behind it,
 * nothing read back.  Neither entry allocates.
 *
 * State (device, the caller's, all zero at the start): ring [streams * track_slots][T][17][3] fp32 and count [streams * track_slots] int64 as the stream
 * entries above keep them, owner [streams * track_slots] int32 = the track id whose history the slot holds (0: nobody's).  Entry g = b * track_slots + s belongs
 * to tracker slot s of stream b.  width, height [streams] fp32, positive: one resolution per STREAM.  resample_tab, first_pos_tab: kasf_stream_tables' tables.
 *
 * The tick rule.  ids, slot, born [streams][track_slots] int32 and count_b [streams] int32 are kasf_sort_update's outputs of this tick (read in place), frames
 * [streams * R][17][3] fp32 the new keypoint frame of every row (H36M-17 pixels + confidence; only read).  count_b is clamped to [0, track_slots].  Row k (k < R)
 * of stream b takes track row
 *     r = count_b - 1 - k   with rows_mode = KASF_ROWS_PERSONS (the k-th oldest emitted track: the row order of kasf_sort_update's persons), or
 *     r = k                 with rows_mode = KASF_ROWS_TRACKS  (the row order of its boxes).
 * The row is VALID iff k < min(count_b, R), id = ids[b][r] >= 1, s = slot[b][r] is in [0, track_slots), and no lower row of the same stream that passes these
 * three tests has the same s (the tracker never emits such duplicates; with hand-made arrays the lowest row wins, the others are invalid).
 * For a valid row, with g = b * track_slots + s:
 *   1. if owner[g] != id or born[b][r] != 0, a new player has the slot: count[g] = 0, owner[g] = id;
 *   2. the frame is stored at ring[g][count[g] % T];
 *   3. count[g] += 1;
 *   4. the row's window is the slot's last L = min(count[g], T) frames, its clips and its pose exactly what kasf_stream_windows and kasf_stream_emit (n_out = 1)
 *      give for a slot with that ring and count at the stream's resolution: the pose is frame max(L - 1 - back, 0) of the window's lift.
 * A track that is not emitted on a tick gets no frame that tick; its history goes on when it comes back under the same id.  A finished track's slot is left as
 * it is: the next id on that slot starts it again.  Ids restart at 1 when the tracker's state is zeroed, so count and owner of those streams must be zeroed
 * with it.  An INVALID row touches no state; its clips are all zero, its pose row is all zero, and valid, ids_out and frames_out are 0.
 *
 * kasf_stream_track_front: one launch, one workgroup per row: resolves the row, applies steps 1-3 and writes x_out [(1 + flip) * streams * R][T][17][3], clip
 * h * streams * R + row, h = 1 the mirrored copy, bit for bit kasf_stream_windows' arithmetic; row_slot [streams * R] int32 receives g, or -1 for an invalid row.
 * Valid rows have distinct g, so no two workgroups touch one state entry: no atomics, the same bits from run to run.  Every index formed from a device value
 * (count_b, slot, count, a table entry) is clamped into the arrays streams, track_slots, R and T describe.
 * kasf_stream_track_emit: out [n_rows][17][3] from the model's output pred [(1 + flip) * n_rows][T][17][3] in the clip order above, merged as kasf_stream_emit
 * merges with n_out = 1; valid [n_rows] uint8 (1 / 0), ids_out [n_rows] int32 (owner[g]), frames_out [n_rows] int64 (count[g], after the push); zeros for
 * rows with row_slot < 0.  row_slot must be what kasf_stream_track_front wrote for this state: its entries index count and owner as they are.
 *
 * n_rows = 0 does nothing.  Error 2, before a device or a device pointer is touched: T outside [1, 256]; streams < 1; track_slots outside 1..64; R < 1;
 * streams * R or streams * track_slots beyond 32 bits; a rows_mode that is neither constant; back outside [0, T - 1]; n_rows < 0; a null pointer. */
#define KASF_ROWS_PERSONS 0
#define KASF_ROWS_TRACKS 1
int kasf_stream_track_front(const float* frames, const int32_t* ids, const int32_t* slot, const int32_t* born, const int32_t* count_b, int32_t streams,
                            int32_t track_slots, int32_t rows_mode, int32_t R, int32_t T, float* ring, int64_t* count, int32_t* owner, const float* width,
                            const float* height, const int32_t* resample_tab, int32_t flip, float* x_out, int32_t* row_slot, void* stream);
int kasf_stream_track_emit(const float* pred, int32_t flip, const int64_t* count, const int32_t* owner, const int32_t* row_slot, int32_t n_rows, int32_t T,
                           const int32_t* first_pos_tab, int32_t back, float* out, uint8_t* valid, int32_t* ids_out, int64_t* frames_out, void* stream);

/* ---- steady keypoints and poses over time: the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) with its state on the device (ADDED under ABI 12:
 * additive, kasf_version() stays 12; look the three symbols up by name).  What ties one tick to the next: in front of the lift over the 2-D keypoints, behind it
 * over the 3-D poses; score-gated, so an occluded joint holds its last estimate.  One launch per call, nothing read back, nothing allocated.
 *
 * A ROW is one person's frame [J][Ct] fp32: the C filtered channels first and, with has_score, one more channel, the score: Ct = C + 1; without it Ct = C.
 * Keypoints are J = 17, C = 2, has_score = 1; poses are J = 17, C = 3, has_score = 0.
 *
 * State per slot g (device, the caller's): xhat [S][J][C] fp32, dxhat [S][J][C] fp32, last [S][J] int64 = the tick of the joint's last update, -1 for none (the
 * initial state is all -1; xhat and dxhat need no initial value), and for the tracked entry owner [S] int32, initially 0, S = streams * track_slots.
 *
 * Parameters (host values, passed by value into the launch): dt (seconds per tick), min_cutoff, d_cutoff (Hz), beta, min_score, max_hold (ticks), and tick, an
 * int64 the caller increases by one per push.  They are in the units of the data: pixels for keypoints, model units for poses.
 *
 * The rule, per joint j of a pushed row x with slot g, in fp32, every line one rounded operation (a line with two: left to right) in this order; the library is
 * built with -ffp-contract=off and a correctly rounded divide:
 *   1. m[c] = x[j][c].  The joint is USABLE iff every m[c] is finite, |m[c]| <= 1e12f, and (with a score) x[j][C] >= min_score; a NaN score fails the comparison.
 *   2. k = max(tick - last[g][j], 1).  If last[g][j] >= 0 and k - 1 > max_hold the estimate is dropped: last[g][j] is treated as -1.
 *   3. No estimate: if the joint is usable, xhat = m, dxhat = 0, last = tick.  Either way the output is the input as it came.
 *   4. Estimate, joint not usable: the output is xhat (hold).  The state is untouched, so k keeps growing.
 *   5. Estimate, joint usable, per channel, with two_pi = 6.2831855f:
 *        dtj  = float(k) * dt
 *        d    = (m - xhat) / dtj
 *        rd   = two_pi * d_cutoff * dtj
 *        ad   = rd / (rd + 1)
 *        dx   = dxhat + ad * (d - dxhat)
 *        fc   = min_cutoff + beta * |dx|
 *        r    = two_pi * fc * dtj
 *        a    = r / (r + 1)
 *        xnew = xhat + a * (m - xhat)
 *      xhat = xnew, dxhat = dx, last = tick; the output is xnew.
 *   6. The score channel is copied through unchanged in every case.
 * The incremental form xhat + a * (m - xhat) reproduces a constant input exactly and returns the first sample as it is.
 *
 * kasf_one_euro_push: x, out [K][J][Ct]; row i goes to slot slots[i] (device int32 [K]), slots = NULL means slot i (K == S) as in kasf_stream_push.  The ids of
 * a call are distinct; an id outside [0, S) makes the row a copy-through that touches no state.
 *
 * kasf_one_euro_tracked: x, out [streams * R][J][Ct]; ids, slot, born [streams][track_slots] int32 and count_b [streams] int32 are kasf_sort_update's outputs of
 * this tick, read in place.  Row k of stream b is resolved by the tick rule of kasf_stream_track_front above -- its track row r, whether it is VALID, its entry
 * g = b * track_slots + s and step 1's test are stated there, once, and computed by the same code.  When step 1's test holds the slot restarts -- every
 * last[g][:] = -1, owner[g] = id -- and then the rule above runs.  An invalid row touches no state and is copied through.  row_slot [streams * R] int32 (may be
 * NULL) receives g, or -1.
 *
 * kasf_one_euro_tracks: recorded tracks packed as x, out [N][J][Ct], track t = rows offsets[t] .. offsets[t + 1] - 1 (device int64 [P + 1], as
 * kasf_lift_windows_ragged takes them; clamped into [0, N]).  Each track starts from an empty state and tick = frame index within the track; the state stays in
 * registers, one launch, and the result equals kasf_one_euro_push called frame by frame bit for bit.
 *
 * One wavefront per row or track; valid rows have distinct g, so there are no atomics, the bits are the same from run to run, and a row's result does not depend
 * on the other rows of the launch.  Every index formed from a device value is clamped.  x and out do not overlap; the inputs are never written.
 *
 * K = 0 / P = 0 does nothing.  Error 2, before a device or a device pointer is touched: J outside [1, 256] or C outside [1, 4]; K or S negative, K > S, NULL
 * slots with 0 < K < S; P or N negative; streams < 1, track_slots outside 1..64, R < 1, streams * R or streams * track_slots beyond 32 bits, a rows_mode that is
 * neither constant; dt, min_cutoff or d_cutoff not in [1e-6, 1e6]; beta not in [0, 1e6]; a non-finite min_score; max_hold outside [0, 2^20]; a negative tick;
 * a null pointer (params included; slots and row_slot may be NULL). */
typedef struct kasf_one_euro_params {
    float dt, min_cutoff, d_cutoff, beta, min_score;
    int32_t max_hold;
} kasf_one_euro_params;
int kasf_one_euro_push(const float* x, const int32_t* slots, int32_t K, int32_t S, int32_t J, int32_t C, int32_t has_score, const kasf_one_euro_params* params,
                       int64_t tick, float* xhat, float* dxhat, int64_t* last, float* out, void* stream);
int kasf_one_euro_tracked(const float* x, const int32_t* ids, const int32_t* slot, const int32_t* born, const int32_t* count_b, int32_t streams,
                          int32_t track_slots, int32_t rows_mode, int32_t R, int32_t J, int32_t C, int32_t has_score, const kasf_one_euro_params* params,
                          int64_t tick, float* xhat, float* dxhat, int64_t* last, int32_t* owner, float* out, int32_t* row_slot, void* stream);
int kasf_one_euro_tracks(const float* x, const int64_t* offsets, int64_t N, int32_t P, int32_t J, int32_t C, int32_t has_score,
                         const kasf_one_euro_params* params, float* out, void* stream);

/* ---- recorded tracks: gaps filled and a zero-phase smoothing (ADDED under ABI 12: additive, kasf_version() stays 12; look the symbol up by name).  A recorded
 * track knows the frames after a gap, which the causal One-Euro filter cannot use: a joint that is not usable is interpolated between its usable neighbours
 * instead of held, and the smoother is symmetric, so it does not lag.  Nothing is read back, nothing is allocated, no atomics: the same bits from run to run.
 *
 * Rows are the One-Euro entries' rows [J][Ct], Ct = C + has_score.  Tracks are packed as x, out [N][J][Ct]; track p = rows offsets[p] .. offsets[p + 1] - 1 =
 * [lo, hi) (device int64 [P + 1], ascending; clamped into [0, N] and to a non-negative length exactly as kasf_one_euro_tracks clamps them: lo = clamp(offsets[p],
 * 0, N), hi = clamp(offsets[p + 1], lo, N)).  A frame n belongs to the last track whose lo is <= n, if n < its hi.  A track never sees another track's frames.
 *
 * Parameters (host values, passed by value into the launch): min_score, max_gap in [0, 64] frames, radius in [0, 32] frames and weights[33], weights[k] = w[k]
 * the weight at distance k frames; entries above radius are ignored.  The kernel calls no transcendental: the weights are the host's (a Gaussian in
 * kasportsformer_amd/refine.py; any non-negative table with w[0] > 0 is taken).
 *
 * The rule, per (track, joint j), in fp32, every line one rounded operation (a line with two: left to right); the library is built with -ffp-contract=off and a
 * correctly rounded divide:
 *   1. Joint j of frame n is USABLE by step 1 of the One-Euro rule above, the same code: every one of its C values satisfies |v| <= 1e12f (a NaN fails) and, with
 *      a score, x[n][j][C] >= min_score (a NaN fails).
 *   2. Fill.  A frame that is not usable has a = the nearest usable frame of joint j in [lo, n) and b = the nearest in (n, hi), where they exist.  Its STATE:
 *        0 usable        the joint is usable:                                                      y = x
 *        1 interpolated  a and b exist and b - a - 1 <= max_gap:   t = float(n - a) / float(b - a);  y[c] = x[a][c] + (x[b][c] - x[a][c]) * t
 *        2 held          a leading run, no usable frame in [lo, n), and b - lo <= max_gap:          y = x[b]
 *                        a trailing run, no usable frame in (n, hi), and hi - 1 - a <= max_gap:      y = x[a]
 *        3 left          everything else (a track without a usable frame included):                 the joint is UNKNOWN, y is not used
 *      A joint of state 0, 1 or 2 is KNOWN.  States 1 and 2 need every frame of the run to be within max_gap frames of n, so every search reaches at most
 *      max_gap frames each way and stops at the track's end; max_gap = 0 fills nothing.
 *   3. Smooth, for a known joint: r = min(radius, n - lo, hi - 1 - n) -- the window is symmetric, so the ends of a track get a narrower window, never a
 *      one-sided one.  num[c] = 0, den = 0; for k = -r .. r ascending with m = n + k, if joint j of frame m is known:
 *        num[c] = num[c] + w[|k|] * (y[m][c] - y[n][c])       (subtract, multiply, add)
 *        den    = den + w[|k|]
 *      and the output is y[n][c] + num[c] / den.  w[0] > 0 and frame n itself is known, so den > 0.  The incremental form returns a constant input bit for
 *      bit and the first and last frame of a track as they are (r = 0); on a linear ramp of known joints the symmetric terms cancel.  radius = 0 smooths
 *      nothing: the output is the filled y.
 *   4. An unknown joint is copied through bit for bit.  The score channel is copied through in every case (a filled joint keeps its low score).
 *   5. state [N][J] uint8 (may be NULL) receives 0 / 1 / 2 / 3 per joint.
 *   6. Rows of x outside every track are not written, in out and in state, as in kasf_one_euro_tracks.
 *
 * kasf_tracks_refine: one launch; a workgroup owns a tile of consecutive packed frames (which may span several short tracks) and a chunk of joints, with the
 * filled y of the tile and of radius frames either side in LDS; no intermediate in global memory.  Every index formed from a device value (the offsets) is
 * clamped; with offsets that do not ascend every access still stays inside the arrays, which rows are written is then unspecified.  A track's result does not
 * depend on the other tracks of the launch.  x is only read; out and state do not overlap x.
 *
 * P = 0 or N = 0 does nothing.  Error 2, before a device or a device pointer is touched: J outside [1, 256] or C outside [1, 4]; P or N negative; max_gap outside
 * [0, 64]; radius outside [0, 32]; a non-finite min_score; a weight of weights[0 .. radius] that is not finite, is negative or is above 1e6; weights[0] not > 0; a null
 * pointer (params included; state may be NULL). */
typedef struct kasf_refine_params {
    float min_score;
    int32_t max_gap, radius;
    float weights[33];
} kasf_refine_params;
int kasf_tracks_refine(const float* x, const int64_t* offsets, int64_t N, int32_t P, int32_t J, int32_t C, int32_t has_score, const kasf_refine_params* params,
                       float* out, uint8_t* state, void* stream);

/* ---- constant limb lengths per player (ADDED under ABI 12: additive, kasf_version() stays 12; look the four symbols up by name).  The lift predicts every
 * window on its own and the One-Euro filter steadies positions, not the skeleton: a thigh still breathes from frame to frame.  This stage, between the lift and
 * kasf_pose_world, gives every bone of a player one length and re-imposes it on every frame, keeping the directions (so the joint angles) and the root.
 * Nothing is read back, nothing is allocated, floating-point atomics are not used: the bits are the same from run to run.
 *
 * A FRAME is [17][3] fp32 in the Human3.6M order.  BONE k (0..15) joins child joint k + 1 to parent joint (0,1,2,0,4,5,0,7,8,9,8,11,12,8,14,15)[k] (the model's
 * own table, get_limb_lens of utils/loss_calc.py); a parent has the lower index, so ascending k walks from the root.
 *
 * The rule, in fp32, every line one rounded operation (a line with two: left to right); the library is built with -ffp-contract=off and a correctly rounded
 * divide and square root:
 *   1. Length of bone k in a frame x:  v = x[child] - x[parent];  l = sqrtf((vx * vx + vy * vy) + vz * vz).  The length is USABLE iff l is finite and l > 0.
 *      A frame is USABLE iff all its 51 values are finite.
 *   2. Target length of a track: L[p][k] = the lower median of the usable lengths of bone k over the usable frames of track p, the element of rank
 *      (n - 1) / 2 (integer division) in ascending order; cnt[p][k] = n; n = 0 gives L = 0, which means "leave this bone alone".  An entry of a table that is
 *      not > 0 means the same.  An order statistic: its bits do not depend on how it is found.
 *   3. symmetric: the left / right partner bones 0-3, 1-4, 2-5, 10-13, 11-14, 12-15 each get (La + Lb) * 0.5f; if one of the two is 0, both get the other.
 *      Applied to the table before use, never stored; applying it twice gives the same bits.
 *   4. Apply, per usable frame: y[0] = x[0]; for k ascending: if L[k] > 0 and l is usable, s = L[k] / l and y[child] = y[parent] + v * s (multiply, then add);
 *      otherwise y[child] = y[parent] + v.  A frame that is not usable is copied through bit for bit.
 *   5. Live: per slot g, len [S][16] fp32 and cnt [S][16] int32 (initially cnt = 0; len needs no initial value).  A usable frame updates every usable bone:
 *      if cnt == 0, len = l, otherwise len = len + (l - len) / float(min(cnt + 1, window)); then cnt = min(cnt + 1, window): the running mean over the first
 *      `window` frames, after that an exponential average of weight 1 / window.  The frame is then walked by 4 with the table L[k] = cnt > 0 ? len : 0, after 3
 *      if symmetric.  A frame that is not usable, or an invalid row, is copied through and leaves len and cnt as they are.  The live form is a mean, not a median.
 *
 * kasf_bone_median: poses [N][17][3] packed, track p = frames offsets[p] .. offsets[p + 1] - 1 (device int64 [P + 1], clamped into [0, N] and to a non-negative
 * length as kasf_one_euro_tracks clamps them) -> lengths [P][16] fp32 and, unless NULL, counts [P][16] int32.  scratch: N * 16 floats of the caller's (the
 * lengths, bone-major).  Two launches: the lengths over the packed frames, then a radix select over their bit patterns, one workgroup per (track, bone).
 *
 * kasf_bone_apply: poses, out [N][17][3].  per_track != 0: lengths [P][16] and offsets [P + 1], which must ascend from 0 to N (as the median's do); a frame of no
 * track is copied through.  per_track == 0: lengths is one [16] for every frame, offsets and P are not read.  One launch; out and poses are distinct arrays.
 *
 * kasf_bone_push: poses, out [K][17][3]; row i goes to slot slots[i] (device int32 [K]), slots = NULL means slot i (K == S), as kasf_one_euro_push.  The ids of
 * a call are distinct; an id outside [0, S) makes the row a copy-through that touches no state.  One launch, one wavefront per row.
 *
 * kasf_bone_tracked: poses, out [streams * R][17][3]; ids, slot, born, count_b, rows_mode, R, owner [streams * track_slots] (initially 0) and row_slot (may be
 * NULL) are kasf_one_euro_tracked's, and a row's slot, validity and restart are resolved by the tick rule of kasf_stream_track_front, as there (stated once,
 * computed by the same code).  A slot that restarts gets cnt[g][:] = 0 and
 * owner[g] = id whatever the frame holds; then rule 5 runs.
 *
 * P = 0 (median), N = 0 (apply) or K = 0 does nothing.  Error 2, before a device or a device pointer is touched: N or P negative, N >= 2^31; K or S negative,
 * K > S, NULL slots with 0 < K < S; window outside [1, 2^20]; streams < 1, track_slots outside 1..64, R < 1, streams * R or streams * track_slots beyond 32
 * bits, a rows_mode that is neither constant; out == poses (apply); a null pointer (counts, slots and row_slot may be NULL; offsets with per_track == 0;
 * poses and scratch of the median with N == 0).  The inputs are never written. */
int kasf_bone_median(const float* poses, const int64_t* offsets, int64_t N, int32_t P, float* scratch, float* lengths, int32_t* counts, void* stream);
int kasf_bone_apply(const float* poses, const int64_t* offsets, int64_t N, int32_t P, const float* lengths, int32_t per_track, int32_t symmetric, float* out,
                    void* stream);
int kasf_bone_push(const float* poses, const int32_t* slots, int32_t K, int32_t S, int32_t window, int32_t symmetric, float* len, int32_t* cnt, float* out,
                   void* stream);
int kasf_bone_tracked(const float* poses, const int32_t* ids, const int32_t* slot, const int32_t* born, const int32_t* count_b, int32_t streams,
                      int32_t track_slots, int32_t rows_mode, int32_t R, int32_t window, int32_t symmetric, float* len, int32_t* cnt, int32_t* owner, float* out,
                      int32_t* row_slot, void* stream);

/* ---- lifted poses placed in camera space (ADDED under ABI 12: additive, kasf_version() stays 12; look the symbol up by name).  The lift returns every pose
 * root-relative, joint 0 at the origin, so every player stands on the same spot.  With the 2-D keypoints the pose came from and the camera's intrinsics, the
 * root translation T that makes the pose re-project onto its keypoints is a 3 x 3 linear least-squares problem per frame; this stage solves it on the device.
 * Frames are independent of one another: a recorded track and one live tick are the same call.  Nothing is read back, nothing is allocated, no atomics: the
 * same bits from run to run.  The camera is a pinhole, (fx, fy, cx, cy) in pixels: THERE IS NO DISTORTION MODEL HERE; undistort the keypoints first where the lens
 * needs it (kasf_keypoints_undistort below).
 *
 * Per frame: the pose P [17][3] fp32, root-relative, in any one unit; the keypoints k [17][3] fp32, pixel x, pixel y, score, in the Human3.6M-17 layout; the
 * camera (fx, fy, cx, cy) fp32.  ALL ARITHMETIC BELOW IS IN FP64 (on players at 4 - 40 m with f = 1500 px the system's condition number reaches 4e4), joints
 * and bones in ascending order, every line one rounded operation (a line with several: by its parentheses, then left to right); the library is built with
 * -ffp-contract=off and a correctly rounded divide and square root.  An fp32 input enters by an exact conversion; results are rounded to fp32 once, at the store.
 *   1. Joint j is USABLE when its keypoint passes step 1 of the One-Euro rule above with C = 2 and a score, the same code (|x|, |y| <= 1e12f and score >=
 *      min_score; a NaN fails) and its three pose values are finite.  n = the number of usable joints.
 *   2. scale.  Without a bone table, scale = 1.  With a table L [16] fp32 in metres (bone b joins joint b + 1 to its parent, kasf_bone_median's table; an entry
 *      that is not > 0 means "skip this bone"): sumL = 0, sumP = 0; for b ascending with L[b] > 0: d = P[b + 1] - P[parent(b)];
 *      sumL = sumL + L[b]; sumP = sumP + sqrt((dx * dx + dy * dy) + dz * dz); then scale = sumL / sumP.  p[j] = P[j] * scale for every joint.  The model's unit is
 *      image pixels, so a player's size in pose units changes with depth: the scale is per frame.  (The other route to metres: kasf_bone_apply with the table
 *      first, then this entry without one.)  A table with no entry > 0 gives 0 / 0, which is state 3.
 *   3. The fit.  Weights w0[j] = score[j] when weighted, else 1; w = w0 in pass 0.  S = Sx = Sy = Sq = b0 = b1 = b2 = 0; for each usable j ascending:
 *        xh = (u - cx) / fx;  yh = (v - cy) / fy;  q1 = xh * pz - px;  q2 = yh * pz - py        (the rows [1, 0, -xh] T = q1 and [0, 1, -yh] T = q2)
 *        S = S + w;  Sx = Sx + w * xh;  Sy = Sy + w * yh;  Sq = Sq + w * (xh * xh + yh * yh)
 *        b0 = b0 + w * q1;  b1 = b1 + w * q2;  b2 = b2 + w * (xh * q1 + yh * q2)
 *      The normal matrix is A = [[S, 0, -Sx], [0, S, -Sy], [-Sx, -Sy, Sq]] with the right-hand side (b0, b1, -b2).  It is solved by eliminating the first two
 *      unknowns (Cholesky's pivots without the square roots):
 *        D = Sq - (Sx * Sx + Sy * Sy) / S
 *        Tz = ((Sx * b0 + Sy * b1) / S - b2) / D;  Tx = (b0 + Sx * Tz) / S;  Ty = (b1 + Sy * Tz) / S
 *      THE PIVOT TEST: A counts as positive definite when S > 0 and D > 1e-9 * Sq (a NaN fails): keypoints that spread over less than about 3e-5 of the
 *      focal length, a twentieth of a pixel at f = 1500, do not fix a depth.
 *   4. Re-weighting, `iterations` times (in [0, 8]): for each usable j: X = px + Tx, Y = py + Ty, Z = pz + Tz;
 *        du = (fx * (X / Z) + cx) - u;  dv = (fy * (Y / Z) + cy) - v;  r2 = du * du + dv * dv;  w = w0 / (1 + r2 / (delta * delta))
 *      (Cauchy weights: no square root), then step 3's sums and solve again with these w.  delta is in pixels; delta * delta is the product of the two fp32
 *      values in fp64.
 *   5. Outputs, with r2 of step 4 at the final T:  num = num + w0 * r2 and den = den + w0 over the usable joints;
 *        out[j] = fp32(P[j] * scale + T) for all 17 joints (a joint whose pose value is not finite stays not finite),  root = fp32(T),
 *        residual = fp32(sqrt(num / den)) in pixels,  scale = fp32(scale), stored whatever the state.
 *   6. state, uint8, the first that applies:
 *        1  n < min_joints (min_joints in [2, 17])
 *        3  scale is not finite and positive (a pose value that is not finite on a bone of the table, a table without an entry > 0, coincident joints)
 *        2  a degenerate fit: in any pass the pivot test fails, or Tx, Ty or Tz is not finite, or a usable joint has Z = pz + Tz <= 0 at any T
 *        0  placed
 *      A frame whose state is not 0 gets NaN (0x7fc00000) in all of out, in root and in residual: kasf_tracks_refine over the roots (has_score = 0) then
 *      interpolates it from its neighbours.
 *
 * kasf_pose_place: poses, keypoints, out [frames][17][3]; camera one row [4] for every frame, or with camera_per_frame != 0 [frames][4]; lengths NULL for no
 * table, one row [16], or with lengths_per_frame != 0 [frames][16]; root [frames][3], residual [frames], scale [frames] and state [frames] may each be NULL.
 * All device pointers.  One launch: a workgroup stages a tile of 64 frames of both inputs in LDS (float4 where poses, keypoints and out are 16-byte aligned),
 * one lane owns one frame with its accumulators in fp64 registers, the placed pose leaves as whole rows.  The inputs are only read; out is an array of its own.
 *
 * frames = 0 does nothing.  Error 2, before a device or a device pointer is touched: frames negative; a non-finite min_score; weighted neither 0 nor 1;
 * iterations outside [0, 8]; delta not finite or not > 0; min_joints outside [2, 17]; out == poses or out == keypoints; a null pointer (params included;
 * lengths, root, residual, scale and state may be NULL).  The defaults of kasportsformer_amd/place.py (min_score 0.3, weighted, 4 iterations, delta 3 px,
 * 4 joints) are a starting point, not tuned on footage. */
typedef struct kasf_place_params {
    float min_score;
    int32_t weighted, iterations;
    float delta;
    int32_t min_joints;
} kasf_place_params;
int kasf_pose_place(const float* poses, const float* keypoints, int64_t frames, const float* camera, int32_t camera_per_frame, const float* lengths,
                    int32_t lengths_per_frame, const kasf_place_params* params, float* out, float* root, float* residual, float* scale, uint8_t* state,
                    void* stream);

/* ---- keypoints of several calibrated cameras -> joints in the world frame, and the lens undistortion (ADDED under ABI 12: additive, kasf_version() stays 12;
 * look the symbols up by name).  A player tracked in C synchronised, calibrated cameras has C keypoint tracks; this stage triangulates them, point by point --
 * one joint of one frame --, on the device.  Points are independent of one another: a recorded track and one live tick are the same call.  Nothing is read
 * back, nothing is allocated, no atomics: the same bits from run to run.  Calibration and synchronisation are the caller's; which tracks are one player: kasf_match_* below.
 *
 * THE CAMERA MODEL, stated once (csrc/camera_model.h).  A camera is 21 fp32 values: fx, fy, cx, cy in pixels; k1, k2, p1, p2, k3, the Brown-Conrady
 * coefficients in OpenCV's order; R [9] row-major and t [3] with X_cam = R X_world + t.  ALL ARITHMETIC BELOW IS IN FP64, views in ascending order, every line
 * one rounded operation (a line with several: by its parentheses, then left to right); the library is built with -ffp-contract=off and a correctly rounded
 * divide and square root.  An fp32 input enters by an exact conversion; results are rounded to fp32 once, at the store.
 *   Normalise:  xd = (u - cx) / fx;  yd = (v - cy) / fy.
 *   Undistort:  x = xd, y = yd, then n times (n = undistort_iterations in [0, 20]; a fixed count with no convergence test, so that the bits do not depend on
 *               the data's path; 0 is a pinhole):
 *                 r2 = x * x + y * y
 *                 rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
 *                 dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
 *                 dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
 *                 x = (xd - dx) / rad;  y = (yd - dy) / rad
 *               With k1 = -0.12, k2 = 0.05, |x| <= 0.6 and f = 1500 px five rounds come within 2e-4 px of the true point and three within 3e-2 px.
 *
 * THE TRIANGULATION RULE, per point seen by C views, 2 <= C <= 16; view c gives the keypoint k = (u, v, score) fp32 and a camera row.
 *   1. View c is USABLE when its keypoint passes step 1 of the One-Euro rule above with C = 2 and a score, the same code (|u|, |v| <= 1e12f and score >=
 *      min_score; a NaN fails) and the 21 values of its camera are finite.  used = the number of usable views, stored whatever the state.  (x, y) of a usable
 *      view is its undistorted point.
 *   2. The fit.  w0 = score when weighted, else 1.  A usable view gives two rows in X, the world point:
 *        a1 = (x * R20 - R00, x * R21 - R01, x * R22 - R02),  r1 = t0 - x * t2        a2 = (y * R20 - R10, y * R21 - R11, y * R22 - R12),  r2 = t1 - y * t2
 *      Pass 0 weights row 1 by wu = w0 * (fx * fx) and row 2 by wv = w0 * (fy * fy): an algebraic error in pixels at unit depth.  The nine sums start at 0 and
 *      take, for each usable view ascending, row 1 and then row 2, with (w, a, r) the row's weight, vector and right-hand side:
 *        A00 = A00 + w * (a0 * a0);  A01 = A01 + w * (a0 * a1);  A02 = A02 + w * (a0 * a2);  A11 = A11 + w * (a1 * a1);  A12 = A12 + w * (a1 * a2)
 *        A22 = A22 + w * (a2 * a2);  b0 = b0 + w * (a0 * r);  b1 = b1 + w * (a1 * r);  b2 = b2 + w * (a2 * r)
 *      The symmetric system A X = b is solved as L D L^T in the order 0, 1, 2 without exchanges:
 *        d0 = A00;  l10 = A01 / d0;  l20 = A02 / d0;  d1 = A11 - l10 * A01;  m12 = A12 - l10 * A02;  l21 = m12 / d1;  d2 = A22 - l20 * A02 - l21 * m12
 *        c1 = b1 - l10 * b0;  c2 = b2 - l20 * b0 - l21 * c1
 *        X2 = c2 / d2;  X1 = c1 / d1 - l21 * X2;  X0 = b0 / d0 - l10 * X1 - l20 * X2
 *      THE PIVOT TEST: d0, d1 and d2 must each be > 1e-9 * (A00 + A11 + A22) (a NaN fails).  Two rays at the angle theta give a least pivot of about
 *      theta^2 / 8 of the trace, so the test fails below 9e-5 rad: a parallax of an eighth of a pixel at f = 1500 px, cameras a millimetre apart at 12 m --
 *      as with kasf_pose_place's 1e-9, the geometry is then below what a keypoint can carry, and fp64 keeps seven digits at that pivot.  It is a floor for the
 *      arithmetic, not a verdict on accuracy: rays a few milliradians apart pass it and fix a depth to metres; `residual` and the rig are the caller's judges.
 *   3. Re-weighting, `iterations` times (in [0, 8]), at the X of the pass before, for each usable view:
 *        Xc = R00 * X0 + R01 * X1 + R02 * X2 + t0;  Yc and Zc with rows 1 and 2 of R and t1, t2;  a usable view with !(Zc > 0) marks the point BEHIND
 *        du = fx * (Xc / Zc - x);  dv = fy * (Yc / Zc - y);  rho = du * du + dv * dv          (pixels of the undistorted image, squared)
 *        g = w0 / (1 + rho / (delta * delta));  wu = g * (fx * fx) / (Zc * Zc);  wv = g * (fy * fy) / (Zc * Zc)
 *      then step 2's sums and solve with these weights: Hartley and Zisserman's iteratively re-weighted linear triangulation -- dividing by the depth turns
 *      the algebraic error into pixels -- with kasf_pose_place's Cauchy weight, which takes a view that does not fit, a swapped joint for instance, out.
 *      delta is in pixels; delta * delta is the product of the two fp32 values in fp64.  With two views nothing tells which of them is wrong: the re-weighting
 *      cannot help there, only the residual shows it.  The sums run in view order, so permuting the views may change the last bits.
 *   4. One more pass only measures, at the final X: rho per usable view as in step 3 (its Zc is tested as well); num = num + w0 * rho and den = den + w0;
 *        residual = fp32(sqrt(num / den)) in pixels;  view_residual[c] = fp32(sqrt(rho)), NaN for a view that is not usable;  points = fp32(X).
 *   5. state, uint8, the first that applies:
 *        1  used < min_views (min_views in [2, 16])
 *        2  degenerate: in any pass a pivot fails the test (rays that do not spread) or X0, X1 or X2 is not finite
 *        3  behind: a usable view has !(Zc > 0) at the X of any pass
 *        0  triangulated
 *      A point whose state is not 0 gets NaN (0x7fc00000) in points, in residual and in every view_residual: kasf_tracks_refine over the points (has_score = 0)
 *      then interpolates it from its neighbours on a recorded track.
 *
 * kasf_keypoints_triangulate: keypoints [views][M][3], M = frames * points_per_frame points in frame-major order; cameras [views][21] for a static rig, or with
 * cameras_per_frame != 0 [views][M / points_per_frame][21] for moving cameras; points [M][3]; residual [M], used [M], state [M] and view_residual [views][M]
 * may each be NULL.  All device pointers.  One launch: one lane per point, a workgroup stages the 128 records of a tile view by view in LDS (float4 where the
 * view's tile is 16-byte aligned), undistorts them once and walks the views out of LDS with its sums in fp64 registers; the points leave as whole rows.  The
 * inputs are only read; points is an array of its own.
 * kasf_keypoints_undistort: keypoints, out [M][3], pixels in, undistorted pixels out: u' = fp32(fx * x + cx), v' = fp32(fy * y + cy) with `iterations` rounds;
 * the score is copied.  camera is the first nine values of a row, [9], or with camera_per_frame != 0 [M / points_per_frame][9].  A point that is not usable
 * -- |u| or |v| not <= 1e12f (one_euro.h's test without a score), or a camera value that is not finite -- is copied as it came.  out is an array of its own.
 *
 * M = 0 does nothing.  Error 2, before a device or a device pointer is touched: views outside [2, 16]; M negative or not a multiple of points_per_frame;
 * points_per_frame < 1; a non-finite min_score; weighted neither 0 nor 1; iterations outside [0, 8]; delta not finite or not > 0; min_views outside [2, 16];
 * undistort_iterations (iterations of the undistortion) outside [0, 20]; points == keypoints, out == keypoints; a null pointer (params included; residual,
 * used, state and view_residual may be NULL).  The defaults of kasportsformer_amd/triangulate.py (min_score 0.3, weighted, 4 iterations, delta 3 px, 2 views,
 * 5 rounds) are a starting point, not tuned on footage. */
typedef struct kasf_triangulate_params {
    float min_score;
    int32_t weighted, iterations;
    float delta;
    int32_t min_views, undistort_iterations;
} kasf_triangulate_params;
int kasf_keypoints_triangulate(const float* keypoints, int32_t views, int64_t M, int32_t points_per_frame, const float* cameras, int32_t cameras_per_frame,
                               const kasf_triangulate_params* params, float* points, float* residual, uint8_t* used, uint8_t* state, float* view_residual,
                               void* stream);
int kasf_keypoints_undistort(const float* keypoints, int64_t M, int32_t points_per_frame, const float* camera, int32_t camera_per_frame, int32_t iterations,
                             float* out, void* stream);

/* ---- matching players across calibrated cameras (no counterpart in the reference, which is monocular): each camera's tracker emits P rows of keypoint tracks,
 * in its own order and with its own ids; these two entries say which row of which camera is the same player, so that kasf_keypoints_triangulate can be fed
 * without the tracks leaving the device.  Cameras are rows of 21 values as above, a static rig only.
 *
 * THE PAIR RULE (kasf_match_pair_costs), in fp64 with the arithmetic of the triangulation rule above: every operation rounded, in the order the parentheses
 * give and then left to right, no fused multiply-add, a correctly rounded divide and square root; fp32 inputs enter by an exact conversion, the cost is rounded
 * to fp32 once.  keypoints [C][P][N][J][3]: C cameras (2 <= C <= 16), P rows per camera (1 <= P <= 64, padded), N synchronised frames, J joints, (u, v, score).
 *   1. A SAMPLE is one joint of one frame of one row.  It is USABLE by step 1 of the triangulation rule, the same code: |u|, |v| <= 1e12f, score >= min_score
 *      (a NaN fails) and the 21 values of its camera finite.  (x, y) = its undistorted point (`undistort_iterations` rounds).  Its ray, in the world frame:
 *        o = 0 - (R0k * t0 + R1k * t1 + R2k * t2), k = 0, 1, 2   (the camera's centre -R^T t)
 *        d = R0k * x + R1k * y + R2k, k = 0, 1, 2                  (R^T (x, y, 1): the parameter along the ray is the depth in the ray's camera)
 *        f = 0.5 * (fx + fy)
 *   2. For cameras a < b, row p of a and row q of b, and a sample index (frame n, joint j) at which both samples are usable, with (o, d, f) of a written
 *      (oa, a, fa) and of b (ob, b, fb):
 *        w = oa - ob (three components);  aa = a0 * a0 + a1 * a1 + a2 * a2;  bb likewise of b;  ab = a0 * b0 + a1 * b1 + a2 * b2
 *        da = a0 * w0 + a1 * w1 + a2 * w2;  db = b0 * w0 + b1 * w1 + b2 * w2;  det = aa * bb - ab * ab
 *        THE PARALLEL TEST: det > 1e-10 * (aa * bb) (a NaN fails) -- det / (aa * bb) is the squared sine of the angle between the rays, so rays closer than
 *        1e-5 rad are not compared; two cameras with one centre give w = 0, s = t = 0, which the next test refuses.
 *        s = (ab * db - bb * da) / det;  t = (aa * db - ab * da) / det     (the depths of closest approach)
 *        s > 0 and t > 0 and both finite, else the sample is NOT COMPARABLE (a closest approach behind a camera)
 *        g_k = (oa_k + s * a_k) - (ob_k + t * b_k);  g = sqrt(g0 * g0 + g1 * g1 + g2 * g2)        (the gap between the rays, in world units)
 *        e = 0.5 * g * (fa / s + fb / t)                                                          (the gap in pixels at the two depths, averaged)
 *        e finite, else not comparable.
 *   3. The sums of a pair (a, p, b, q) over its comparable samples, wt = score_a * score_b (the fp32 scores' product in fp64) when weighted, else 1:
 *        num = num + wt * min(e, cap);  den = den + wt;  count = count + 1           (cap: the fp32 value in fp64; min(e, cap) is e when e < cap)
 *      THE ORDER: the frames are cut into tiles of 256; a tile's sums start at 0 and take its samples frame by frame, joints ascending within a frame; the
 *      pair's sums start at 0 and take the tiles' sums in ascending order.  The order depends on the sample index alone: not on the grid, not on the other rows
 *      or cameras -- a pair has the same bits when only its two cameras are given -- and the same bits come out run after run (no atomics).
 *   4. samples[a][b][p][q] = count.  cost[a][b][p][q] = fp32(num / den) when count >= min_samples, else +inf.  cost[b][a][q][p] and samples[b][a][q][p] are
 *      the same values with the same bits.  The diagonal blocks a == a are +inf with 0 samples.  A weighted pair whose comparable samples all score 0 is 0 / 0.
 *
 * THE GROUPING RULE (kasf_match_groups) over any cost and samples [C][C][P][P], in one launch of one wavefront; cameras are taken in ascending order, so the
 * result depends on the order of the cameras: the first camera's rows seed the groups, and a player it did not see is only grouped from the camera that first
 * did.  That is a property of the rule, not of the kernel.
 *   A group holds at most one row per camera.  There are none at the start.  For camera c = 0, 1, ...:
 *   1. Row q of c is NON-EMPTY when samples[c][m][q][r] > 0 for some other camera m and some row r: a row that was never comparable with anything -- a padded
 *      row, or a player at whom, over the whole track, no other camera looked at anybody -- stays out, group -1.
 *   2. The cost of non-empty row q to group g, over g's members (m, r), cameras m ascending, that are COMPARABLE with it -- cost[m][c][r][q] finite and
 *      samples[m][c][r][q] > 0:  num = num + samples * cost;  den = den + samples (both fp64, starting at 0);  the cost is num / den, or BIG = 1e9 when g
 *      has no comparable member.
 *   3. The assignment of non-empty rows to groups that makes min(rows, groups) pairs with the least total cost, by the shortest-augmenting-path method of
 *      kasf_sort_update (csrc/assignment.h: rows of the walk = the smaller side, the non-empty rows in ascending order and the groups in ascending order, ties
 *      by the totally ordered key (cost, column already assigned, column)).
 *   4. As in SORT's rule 4 a pair made by the assignment is REJECTED when its cost is >= BIG or > max_cost; an accepted row joins its group.
 *   5. The non-empty rows without a group, in ascending row order, open new groups while fewer than max_groups exist; the rest count in `dropped`, group -1.
 *   group [C][P]: the row's group or -1;  members [max_groups][C]: the group's row in each camera or -1;  views [max_groups]: its number of members (0 for
 *   a group that was never opened);  group_cost [max_groups]: fp32 of the mean, in fp64 in camera order, of the costs at which its rows were accepted, NaN
 *   (0x7fc00000) for a group of one view or none;  count [1]: the groups opened;  dropped [1].
 *
 * kasf_match_workspace_bytes: the bytes kasf_match_pair_costs needs at `workspace` (8-byte aligned; the tiles' sums): 20 * ceil(frames / 256) * C (C - 1) / 2
 * * P * P.  -2 on a refusal.
 * kasf_match_pair_costs: two launches -- the pairs, then the sum over tiles (see csrc/k_match.hip for the kernel's shape: a workgroup stages 16 samples of
 * every row of a camera pair through LDS, undistorts them once and walks up to 256 pairs; no ray is written to global memory).  frames = 0 does nothing and
 * leaves cost and samples as they were.  All device pointers; the inputs are only read.
 * kasf_match_groups: one launch.  Nothing is read back by either.
 *
 * Error 2, before a device or a device pointer is touched: cameras outside [2, 16]; rows outside [1, 64]; frames outside [0, 2^31 - 1]; joints < 1; frames *
 * joints >= 2^31; a non-finite min_score; weighted neither 0 nor 1; cap or max_cost not finite or not > 0; min_samples < 1; undistort_iterations outside
 * [0, 20]; max_groups outside [1, 64]; a workspace that is too small or not 8-byte aligned; a null pointer (params included).  The defaults of
 * kasportsformer_amd/match.py (min_score 0.3, weighted, cap 50 px, min_samples 2 * J, 5 rounds, max_cost 15 px) are a starting point, not tuned: nothing was
 * run on footage.  Not here: synchronising the cameras in time, moving cameras, a stateful live matcher that keeps group ids from tick to tick, and
 * cycle-consistent multi-way matching (this rule is greedy in the camera order). */
#define KASF_MATCH_MAX_CAMERAS 16
#define KASF_MATCH_MAX_ROWS 64
typedef struct kasf_match_params {
    float min_score;
    int32_t weighted;
    float cap;
    int32_t min_samples, undistort_iterations;
} kasf_match_params;
int64_t kasf_match_workspace_bytes(int32_t cameras, int32_t rows, int64_t frames);
int kasf_match_pair_costs(const float* keypoints, int32_t cameras, int32_t rows, int64_t frames, int32_t joints, const float* camera_rows,
                          const kasf_match_params* params, float* cost, int32_t* samples, void* workspace, int64_t workspace_bytes, void* stream);
int kasf_match_groups(const float* cost, const int32_t* samples, int32_t cameras, int32_t rows, float max_cost, int32_t max_groups, int32_t* group,
                      int32_t* members, int32_t* views, float* group_cost, int32_t* count, int32_t* dropped, void* stream);

/* debugging / tests: locate a named activation inside the workspace (see kasf_ws_name()) */
int32_t kasf_ws_entries(const kasf_model* m, int32_t batch, int32_t flags);
int kasf_ws_entry(const kasf_model* m, int32_t batch, int32_t flags, int32_t idx, char* name, int32_t name_cap, int64_t* byte_offset,
                  int64_t* numel, int32_t* elem_kind /* 0: model dtype, 1: fp32, 2: fp64, 3: u32 */);

/* ---- single-operator entry points (tensors of the model dtype are void*; M = tokens) ---- */
/* y = act(LN?(a) W^T + bias): a [M,128], w [N,128] (dtype), N % 128 == 0; ln_g == NULL -> no LayerNorm; act 0 none, 1 tanh */
int kasf_op_linear(int32_t dtype, const void* a, const void* w, const float* bias, void* y, int64_t M, int32_t N, const float* ln_g, const float* ln_b,
                   void* xn_out, int32_t act, void* stream);
/* attention proj + layer scale + residual: out = resid + ls * (a W^T + bias): a, resid, out [M,128] and w [128,128] of dtype; bias, ls [128] fp32.  M <= 0: returns 0,
 * nothing is launched (as every entry of this family) */
int kasf_op_linear_res(int32_t dtype, const void* a, const void* w, const float* bias, const float* ls, const void* resid, void* out, int64_t M, void* stream);
/* modules/mlp.py inside a FormerModule: out = x + ls2 * (GELU(LN(x) W1^T + b1) W2^T + b2) */
/* xn_out (optional; bf16 only): also receives LN(x), which kasf_op_mlp_bwd_fused streams instead of recomputing (what training mode does).
 * ABI 7: with dtype = bf16, w2 [128,512] is IEEE FP16 (torch.float16), not bf16: the forward evaluates GELU in packed fp16 and keeps the hidden
 * activation in fp16 for GEMM2 (v_mfma_f32_16x16x32_f16); x, w1 and out stay bf16.  kasf_pack_weights writes that fp16 copy into the arena itself.
 * RANGE (bf16 mode only): the pre-activation z = LN(x) W1^T + b1 and the fc2 weights pass through fp16, whose largest finite value is 65504: |z| > 65504
 * converts to +-inf (GELU(+inf) = inf, GELU(-inf) = -inf . 0 = NaN where the fp32 form returns x and 0), and a fc2 weight beyond 65504 packs to inf.  LayerNorm'd
 * inputs with trained weights are five orders of magnitude below that; a checkpoint that is not should be run with dtype = fp32 (exact erf GELU, no fp16 anywhere). */
int kasf_op_mlp_fwd(int32_t dtype, const void* x, const float* ln_g, const float* ln_b, const void* w1, const float* b1, const void* w2, const float* b2,
                    const float* ls2, void* out, int64_t M, void* xn_out, void* stream);
int kasf_op_mlp_bwd(int32_t dtype, const void* x, const void* g, const float* ln_g, const float* ln_b, const void* w1, const float* b1,
                    const void* w2t_scaled, const void* w1t, void* hbuf, void* dzbuf, void* g_in, float* dgamma, float* dbeta, int64_t M, void* stream);
/* bf16 only: fused MLP backward (hidden-quarter ownership, weights in registers): data gradient AND both weight gradients.
 * g_in = g + LNbwd(dA); dw1 [512,128] += dZ^T LN(x); db1 [512] += colsum(dZ); dw2_unscaled [128,512] += g^T H;
 * gsum [128] += colsum(g); dgamma/dbeta += LayerNorm parameter gradients.  dapart: 4*M*128 elements of scratch (bf16: the four hidden quarters' dA partials;
 * with KASF_MLP_BWD_DZ=1 in the environment, dZ [M,512] in the same bytes: the second launch then forms dA = dZ W1 itself).
 * partial: scratch of at least ranges * 65536 floats, 16-byte aligned, where tiles = ceil(M / 32), per = ceil(tiles / min(tiles, 64)) and
 * ranges = ceil(tiles / per) <= 64 (64 * 65536 floats cover every M).  It is read as bf16: token range r leaves its share of dW1 as one [512][128] bf16 tile
 * at bf16 element r * 65536 and its share of dW2 as one [128][512] bf16 tile at bf16 element (ranges + r) * 65536; the second launch adds the tiles in a fixed
 * order.  Both forms (dA partials and dZ) use exactly these 2 * ranges tiles: nothing behind them is read or written, and no word of it is a flag.
 * M <= 0: nothing is launched. */
int kasf_op_mlp_bwd_fused(const void* x, const void* xn /* LN(x) from kasf_op_mlp_fwd */, const void* g, const float* ln_g, const void* w1, const float* b1, const void* w2t_scaled,
                          const void* w1t, void* dapart, float* partial, float* dw1, float* dw2_unscaled, float* db1, float* gsum, void* g_in,
                          float* dgamma, float* dbeta, int64_t M, void* stream);
/* dW[N,K] += G^T LN?(X), dbias[N] += colsum(G): G [M,N], X [M,K].  partial: optional fp32 scratch of partial_floats
 * elements (>= 256*128*128 covers every shape of this model): per-split tiles are stored and summed by a second
 * kernel (bitwise reproducible); NULL -> fp32 atomics on dw. */
int kasf_op_wgrad(int32_t dtype, const void* g, int32_t N, const void* x, int32_t K, const float* ln_g, const float* ln_b, float* dw, float* dbias,
                  int64_t M, float* partial, int64_t partial_floats, void* stream);
/* out = [resid] + [out, if accumulate] + LNbwd(dY Wt^T [+ dxn_add]): dY [M,Kd], Wt [128,Kd]; dgamma/dbeta are accumulated into;
 * xn_out (optional, with beta) receives LN(x), the operand of the matching weight-gradient GEMM */
int kasf_op_dgrad_lnbwd(int32_t dtype, const void* dy, int32_t Kd, const void* wt, const void* dxn_add, const void* x, const float* gamma,
                        const void* resid, void* out, int32_t accumulate, float* dgamma, float* dbeta, int64_t M, void* xn_out, const float* beta,
                        void* stream);
/* bf16 only: kasf_op_dgrad_lnbwd with the weight gradient of the same linear in the same launch, finished as a backward stage finishes it: after the call
 * out, dgamma, dbeta (as kasf_op_dgrad_lnbwd, no xn_out) and dw [Kd,128] += dY^T LN(x) are complete.  Five forms, anything else is error 2:
 *   Kd 384 or 128 with resid, no accumulate                        (the qkv / q linears)
 *   Kd 256, no resid, accumulate                                     (the bone kv linear)
 *   Kd 256 with resid, dxn_add and dbias [256] += colsum(dY)         (the GCN's U | V linear)
 *   Kd 128 with resid and proj_o [M,128]                             (the bone q linear carrying the block's output-projection gradient): with G = resid^T proj_o
 *       and c = colsum(resid):  dproj_w [128,128] += proj_ls[n] G[n][:],  dproj_b [128] += proj_ls . c,  dproj_ls [128] += <proj_w[n], G[n]> + proj_b . c;
 *       proj_o, proj_w, proj_b, proj_ls, dproj_w, dproj_b, dproj_ls and proj_part go together.
 * Scratch, all 16-byte aligned: wpart, wpart_bytes >= 256 * Kd * 128 * 2 (bf16 partial tiles of dw, one per workgroup); proj_part, proj_part_bytes >= 256 * 128 * 128 * 2
 * + 256 * 128 * 4 (the proj tiles and behind them one fp32 row of colsum(resid) per workgroup); scratch, scratch_floats >= rows * ld rounded up to 64, rows =
 * the workgroups that own a tile (tiles = ceil(M / 32), per = ceil(tiles / min(tiles, 256)), rows = ceil(tiles / per)), ld = 512 with dbias and 256 without: one row
 * of dgamma | dbeta (| dbias) per workgroup, summed in a fixed order.  M <= 0: returns 0 after the checks, nothing is launched. */
int kasf_op_dgrad_wg(const void* dy, int32_t Kd, const void* wt, const void* dxn_add, const void* x, const float* gamma, const float* beta, const void* resid,
                     void* out, int32_t accumulate, float* dgamma, float* dbeta, float* dw, float* dbias, const void* proj_o, const float* proj_w,
                     const float* proj_b, const float* proj_ls, float* dproj_w, float* dproj_b, float* dproj_ls, int64_t M, void* wpart, int64_t wpart_bytes,
                     void* proj_part, int64_t proj_part_bytes, float* scratch, int64_t scratch_floats, void* stream);
/* bf16 only: up to three weight gradients of one block in one streaming launch and one finishing launch, exactly the launch a backward stage makes for an
 * attention or bone block (and nothing else):  dw[j] [N[j],128] fp32 += g[j]^T x[j],  g[j] [M,N[j]] and x[j] [M,128] bf16 token-major, N[j] in {128, 256, 384, 512},
 * njobs in 1..3; g, x, N, dw and dbias are host arrays of njobs entries.  Each token split leaves one bf16 partial tile per job; the finishing launch adds them in a
 * fixed order.
 *   fin_job (-1, or a job index with N = 128): that job is the layer-scaled proj weight.  With G = g^T x and c = colsum(g):  dw += fin_ls[n] G[n][:],
 *       dls [128] += <fin_w[n], G[n]> + fin_bias[n] c[n],  dbias[fin_job] [128] += fin_ls[n] c[n].  fin_w [128,128], fin_bias, fin_ls, dls and dbias[fin_job] are all
 *       needed; dbias[j] of every other job must be NULL.
 *   nred in 0..2 reductions ride in the finishing launch:  red_out[k][e] += sum over z < red_nparts[k] of red_part[k][z][e], e < red_elems[k] (bf16 parts, a multiple
 *       of 128 elements); red_part, red_out, red_nparts, red_elems are host arrays of nred entries (NULL with nred = 0).
 *   ext_part (optional; needs fin_job = -1 and njobs <= 2): the proj job when its ext_nparts >= 1 partial tiles [128][128] bf16 and rows ext_brow [ext_nparts][128] fp32
 *       (colsum per tile) were left by another kernel: the algebra above with G = sum of the tiles, c = sum of the rows, into ext_dw, dls and ext_db; it needs the four
 *       fin_* vectors.
 *   partial: fp32-typed scratch of partial_floats >= sum over jobs of splits * N[j] * 128 (+ splits * 128 for the fin job), where tiles = sum N[j] / 128,
 *       splits0 = min(ceil(248 / tiles), ceil(M / 128)), slice = ceil(ceil(M / splits0) / 128) * 128 and splits = ceil(M / slice).
 * Every array is 16-byte aligned.  Error 2, nothing launched, in this order: njobs, nred or fin_job out of range; M >= 2^31; a NULL host array; N[j] not one of the four;
 * a NULL or misaligned array; dbias on a job other than fin_job; a fin job with N != 128, or without its vectors or its dbias; ext_part together with fin_job >= 0 or
 * njobs > 2; ext_part without ext_brow, ext_nparts >= 1, ext_dw, ext_db and the fin vectors (or one of those without ext_part); red_nparts < 1 or red_elems not a
 * positive multiple of 128; partial_floats too small (M > 0).  M <= 0 returns 0 after the other checks. */
int kasf_op_wgrad_jobs(int32_t njobs, const void* const* g, const void* const* x, const int32_t* N, float* const* dw, float* const* dbias, int32_t fin_job,
                       const float* fin_w, const float* fin_bias, const float* fin_ls, float* dls, int64_t M, float* partial, int64_t partial_floats, int32_t nred,
                       const void* const* red_part, float* const* red_out, const int32_t* red_nparts, const int32_t* red_elems, const void* ext_part,
                       const float* ext_brow, int32_t ext_nparts, float* ext_dw, float* ext_db, void* stream);
/* attention core (selfattention.py:18-41): q [*,ldq], k/v [*,ldkv] token-major; mode 0 spatial, 1 temporal; o and d_o are [M,128] (leading dimension 128).
 * The five kasf_op_attention_* entries refuse (error 2, nothing launched): a mode other than 0 or 1, batch < 0, n_frames < 1, batch * n_frames * 17 * max(384, the
 * largest leading dimension) >= 2^31 (the kernels index in 32 bits), a leading dimension below 128 (the columns each of q, k, v, dq, dk, dv addresses from its own
 * pointer) or not a multiple of 8 elements, a NULL pointer, and a pointer that is not 16-byte aligned (rows move in 16-byte pieces in both dtypes).  batch = 0
 * returns 0 after the checks and launches nothing (kasf_op_attention_bwd_fused_do refuses batch < 1, as it always did).  Columns between 128 and a padded leading
 * dimension are neither read nor written. */
int kasf_op_attention_fwd(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int32_t batch, int32_t n_frames,
                          int32_t mode, void* stream);
int kasf_op_attention_bwd(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* d_o, void* dq, int64_t lddq,
                          void* dk, void* dv, int64_t lddkv, int32_t batch, int32_t n_frames, int32_t mode, void* stream);
/* the same for num_heads in {2, 4, 8, 16} (head dimension 128 / num_heads; the two entries above are num_heads = 8): bf16 mode runs MFMA cores for 8 and 4 heads
 * (4 = the reference constructor's default, KASportsFormer.py:293) on groups of up to 256 positions, LDS-resident fp32 cores otherwise */
int kasf_op_attention_fwd_heads(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* o, int32_t batch, int32_t n_frames,
                                int32_t mode, int32_t num_heads, void* stream);
int kasf_op_attention_bwd_heads(int32_t dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* d_o, void* dq, int64_t lddq,
                                void* dk, void* dv, int64_t lddkv, int32_t batch, int32_t n_frames, int32_t mode, int32_t num_heads, void* stream);
/* bf16, 8 heads, groups of <= 96 positions: the same with d_o = g_mid . wproj_t_scaled^T formed inside the kernel (what the training step runs:
 * attention.py's proj + layer-scale data gradient folded in); wproj_t_scaled [128 in][128 out] = (ls1 . Wproj)^T packed bf16.
 * Groups of <= 32 positions: form 0 = persistent kernel (the engine's), 1 = one group per workgroup (the comparison point): bit-identical results.
 * Groups of 33..96 positions (temporal attention at T = 81): with o_saved [M,128] (the attention output) and lse [M,8] fp32 (log-sum-exp of the scaled
 * scores per token and head), both as the training forward leaves them, the key-tile-outer kernel runs; with either NULL the self-contained one. */
int kasf_op_attention_bwd_fused_do(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, const void* g_mid, const void* wproj_t_scaled,
                                   void* dq, int64_t lddq, void* dk, void* dv, int64_t lddkv, int32_t batch, int32_t n_frames, int32_t mode, int32_t form,
                                   const void* o_saved, const float* lse, void* stream);
/* bf16, 8 heads, groups of <= 96 positions: the forward of one attention block (bone = 0, selfattention.py:18-41) or bone cross-attention block (bone = 1,
 * bone_crossattention.py:19-41) in one launch, exactly as the engine launches it:
 *     out = x + ls1 * (proj(softmax(q k^T / 4) v) + bproj),   bone 0: q | k | v = LN(x; ln_g, ln_b) wq^T,            wq [384,128] (rows 0..127 q, 128..255 k, 256..383 v)
 *                                                             bone 1: q = LN(x) wq^T, wq [128,128];  k | v = LN(x_limb; lnl_g, lnl_b) wkv^T,  wkv [256,128]
 * x, x_limb, out [M,128] bf16 token-major, M = batch * n_frames * 17 in [batch][frame][joint] order; wq, wkv, wproj [128,128] bf16 row-major [out][in]; the LayerNorm
 * parameters, bproj and ls1 are fp32 [128].  Head h owns features 16h..16h+15 of q, k and v.  mode 0: a group is the 17 joints of a frame; 1: the n_frames
 * positions of one (clip, joint) track.
 * Saves (what a backward pass reads; all NULL in evaluation, when nothing but out is written): q_save [M,384] = q | k | v (bone: [M,128] = q) and o_save [M,128] (the
 * heads' outputs in front of proj) go together; kv_save [M,256] = k | v is given exactly when bone = 1 and the saves are given; lse_save [M,8] fp32 (log-sum-exp of
 * the scaled scores per token and head, the operand of kasf_op_attention_bwd_fused_do's key-tile-outer kernel) is optional with the saves and is written only for
 * groups of 33..96 positions -- for shorter groups it is left untouched.
 * out must not alias x or x_limb: a workgroup loads the next group's rows while it stores.  Every bf16 pointer is 16-byte aligned.
 * Refused with error 2, in this order: bone or mode not 0 / 1; batch < 0; n_frames < 1; batch * n_frames * 17 * 384 >= 2^31; groups of more than 96 positions
 * (mode 1: n_frames > 96); the bone operands (x_limb, lnl_g, lnl_b, wkv) not all given with bone = 1 or not all NULL with bone = 0; the saves not together as above;
 * a NULL among the other pointers; out aliasing an input; a misaligned bf16 pointer.  batch = 0 returns 0 after the checks and launches nothing. */
int kasf_op_attn_block_fwd(int32_t bone, const void* x, const void* x_limb, const float* ln_g, const float* ln_b, const float* lnl_g, const float* lnl_b, const void* wq,
                           const void* wkv, const void* wproj, const float* bproj, const float* ls1, void* q_save, void* kv_save, void* o_save, float* lse_save,
                           void* out, int32_t batch, int32_t n_frames, int32_t mode, void* stream);
/* bf16, 8 heads, groups of <= 32 positions: the backward of one attention block (bone = 0) or bone cross-attention block (bone = 1) from x (, x_limb) and
 * g_mid = d(loss)/d(x_mid) in one launch, finished as the engine finishes it (the streaming weight gradient with the proj job's tiles, then the column sink's flush):
 *   xn_a = LN(x) (bone: xn_b = LN_limb(x_limb)) [M,128];  dq = dq | dk | dv [M,384] (bone: dq [M,128], dkv = dk | dv [M,256]) of the attention core on
 *   q | k | v re-formed from xn and d_o = g_mid wproj_t_scaled^T;  out = g_mid + LNbwd(dq | dk | dv . wq) (bone: out_limb += LNbwd_limb(dk | dv . wkv));
 *   dgamma, dbeta (dgamma_l, dbeta_l) += the LayerNorms' parameter gradients;  dw_mix [384,128] (bone [128,128]; dw_kv [256,128]) += dq^T xn;
 *   with G = g_mid^T o and c = colsum(g_mid):  dproj_w += ls1[n] G[n][:],  dproj_b += ls1 . c,  dls1 += <proj_w[n], G[n]> + proj_b . c.
 * wq: forward layout [384,128] (bone [128,128]), wkv [256,128], wq_t = wq^T [128,128] (bone only), wproj_t_scaled = (ls1 . Wproj)^T [128 in][128 out], all bf16;
 * proj_w [128,128], proj_b, ls1 and the LayerNorm vectors fp32.  The eleven bone arguments (x_limb, lnl_g, lnl_b, wkv, wq_t, out_limb, dkv, xn_b, dgamma_l, dbeta_l,
 * dw_kv) are all given with bone = 1 and all NULL with bone = 0.  out must not alias x or x_limb.
 * Scratch, 16-byte aligned: partial, partial_floats >= splits * 384 * 128 (splits as kasf_op_wgrad_jobs states it, for M = batch * n_frames * 17 and three tiles);
 * proj_part, proj_part_bytes >= 256 * 128 * 128 * 2 + 256 * 128 * 4 (as kasf_op_dgrad_wg); scratch, scratch_floats >= active * (bone ? 512 : 256) rounded up to 64,
 * active = ceil(groups / ceil(groups / min(groups, 256))) workgroups that own a group: with less the call returns error 6 and launches nothing.
 * Error 2 in this order: bone, mode, batch < 0, n_frames < 1, the 2^31 index bound, groups of more than 32 positions, the bone arguments, a NULL pointer, out
 * aliasing an input, alignment, scratch_floats < 1, proj_part_bytes, partial_floats.  batch = 0 returns 0 after the checks. */
int kasf_op_attn_block_bwd(int32_t bone, const void* x, const void* x_limb, const void* g_mid, const float* ln_g, const float* ln_b, const float* lnl_g, const float* lnl_b,
                           const void* wq, const void* wkv, const void* wq_t, const void* wproj_t_scaled, const float* proj_w, const float* proj_b, const float* ls1,
                           void* out, void* out_limb, void* dq, void* dkv, void* xn_a, void* xn_b, float* dgamma, float* dbeta, float* dgamma_l, float* dbeta_l,
                           float* dw_mix, float* dw_kv, float* dproj_w, float* dproj_b, float* dls1, float* partial, int64_t partial_floats, void* proj_part,
                           int64_t proj_part_bytes, float* scratch, int64_t scratch_floats, int32_t batch, int32_t n_frames, int32_t mode, void* stream);
/* ---- the GCN mixer on its own (ABI 12; modules/graph.py:19-134 between the U | V Linear and the residual of KASportsFormer.py:109) ----
 * M = batch * n_frames * 17 tokens in [batch][frame][joint] order.  mode 0 = spatial (fixed skeleton adjacency, BatchNorm channel = joint, 17 nodes), 1 = temporal
 * (per (clip, joint) track: S = xn xn^T, every frame whose similarity reaches the neighbour_num-th largest of its row is a neighbour -- ties are all kept, so a row's
 * degree may exceed neighbour_num --, BatchNorm channel = frame, n_frames nodes).  Both entries run the engine's own launches with the engine's own
 * count = batch * n_frames * 128 (spatial) or batch * 17 * 128 (temporal) values per node.
 *   y    = D^-1/2 A D^-1/2 . V + U          uv [M,256] = U | V of xn, bias included (kasf_op_linear with N = 256)
 *   out  = x_in + ls1 * relu(xn + BN(y))    xn [M,128] = LN(x_in), as kasf_op_linear's xn_out leaves it
 * training != 0: BatchNorm on the batch mean and biased variance of y AS STORED (rounded to the model dtype), and run_mean / run_var become (1 - momentum) * old +
 * momentum * (mean, unbiased variance); training == 0: BatchNorm on run_mean / run_var, which are not written.  mask [batch * 17][n_frames][MW] uint32 receives the
 * temporal adjacency (bit c of word c >> 5 of row r = "frame c is a neighbour of frame r"; MW = 3 up to 96 frames, ceil(n_frames / 32) beyond; NULL in spatial mode).
 * coef [256][8] fp32 receives per node: scale, shift, mean, rstd (4 more floats of scratch).
 * stats / bstats: ONE statistics buffer each, KASF_GCN_STAT_WORDS int64 words, zeroed by the entry itself (hipMemsetAsync on `stream`, as kasf_forward does) and
 * left readable.  Layout [4 slots][512 statistics][5 words]: statistic 2 n of node n is the sum of y (bstats: of r), statistic 2 n + 1 the sum of y^2 (bstats: of
 * r . (y - mean) . rstd).  Words 0..3 are SIGNED counts of units 2^(-110 + 52 k) of one fixed-point number (a negative partial adds two's-complement pieces, each
 * word keeps 12 bits of head room for carries), so a statistic's value is EXACTLY sum_slots sum_{k<4} word[k] 2^(-110 + 52 k): each workgroup adds its fp32 partial
 * sum to slot (workgroup index mod 4) with 64-bit integer atomics, bits below 2^-110 floored toward -inf (at most once per workgroup; grids of at most 1,024
 * workgroups).  Word 4 is the poison flag: non-zero once a partial was non-finite or >= 2^97 in magnitude; readers then take the statistic as NaN.
 * RANGE: the variance is E[y^2] - mean^2 from those two sums, and each workgroup's partial of either is an fp32 sum, so a node whose |mean| / std = rho loses about
 * (1 + rho^2) 2^-22 of its variance relative to a two-pass (torch.nn.BatchNorm1d) evaluation: rho = 8 is held to the 1e-4 / 3e-2 parity bars, rho = 64 to those
 * bars plus twice that sensitivity (tests/test_gpu_gcn.py).  Default-initialised and trained-from-default weights sit at rho < 1 (U and V have zero-mean weights
 * and see LayerNorm'd rows).
 * Error 2, before any device is touched: n_frames outside [4, 256], neighbour_num outside [1, 4], mode not 0 / 1, batch < 1 or batch * n_frames * 17 * 16 >= 2^31,
 * a required pointer that is null. */
#define KASF_GCN_STAT_WORDS (4 * 512 * 5)
int kasf_op_gcn_fwd(int32_t dtype, const void* x_in, const void* xn, const void* uv, const float* bn_w, const float* bn_b, float* run_mean, float* run_var,
                    const float* ls1, void* y, uint32_t* mask, void* stats, float* coef, void* out, int32_t batch, int32_t n_frames, int32_t mode,
                    int32_t neighbour_num, int32_t training, float momentum, void* stream);
/* Gradients of the above for g [M,128] = d/d(out): r [M,128] = ls1 . g where the ReLU passed (the direct d/d(xn) term, and d/d(BN(y))), duv [M,256] = dU | dV (the
 * adjacency carries no gradient); dls1 [128], d_bn_w and d_bn_b [nodes] are ACCUMULATED into.  xn, y, coef and mask as kasf_op_gcn_fwd left them; training as there
 * (0: mean and variance are constants, duv has no batch-mean terms). */
int kasf_op_gcn_bwd(int32_t dtype, const void* g, const void* xn, const void* y, const float* coef, const uint32_t* mask, const float* ls1, void* r, void* duv,
                    float* dls1, float* d_bn_w, float* d_bn_b, void* bstats, int32_t batch, int32_t n_frames, int32_t mode, int32_t training, void* stream);
/* ---- the MLP, data-gradient and GCN backward kernels in the form a backward stage runs them (ADDED under ABI 12: additive, kasf_version() stays 12).  Each entry
 * puts a column sink on the caller's scratch, calls the launcher that kasf_backward calls, and finishes the sink in a fixed order on `stream`: every per-channel
 * sum (dgamma, dbeta, db1, colsum(g), dls1) leaves its kernel as one row per workgroup and is bit-reproducible.  scratch: device floats, 16-byte aligned,
 * scratch_floats >= kasf_op_sink_scratch_floats(...).  Error 2: scratch with scratch_floats < 1 or misaligned, and what the entry without scratch refuses.
 * kasf_op_mlp_bwd_rows, kasf_op_dgrad_lnbwd_rows, kasf_op_gcn_bwd_rows: the parameters and results of kasf_op_mlp_bwd, kasf_op_dgrad_lnbwd and kasf_op_gcn_bwd.  A NULL
 * scratch is that entry (fp32 atomics); a scratch that is too small falls back to the atomics (results still complete) and returns error 6. */
#define KASF_SINK_MLP_BWD_FUSED_FC2 0
#define KASF_SINK_MLP_BWD_ROWS 1
#define KASF_SINK_DGRAD_LNBWD_ROWS 2
#define KASF_SINK_GCN_BWD_ROWS 3
#define KASF_SINK_FORM_RESID 1
#define KASF_SINK_FORM_DXN_ADD 2
#define KASF_SINK_FORM_ACCUMULATE 4
#define KASF_SINK_FORM_XN_OUT 8
/* floats of scratch the entry asks for at M tokens (gcn_bwd_rows: M = batch * n_frames * 17): the sum over the launch's requests of rows * row length, each rounded up to
 * 64 floats.  dtype: of the call (ignored by mlp_bwd_fused_fc2).  Kd and form (KASF_SINK_FORM_* of the operands given) are read for dgrad_lnbwd_rows only: they
 * decide which kernel runs.  -2 with kasf_last_error() set: M < 1, unknown op, bad dtype, Kd not a multiple of 128.  Needs no device. */
int64_t kasf_op_sink_scratch_floats(int32_t op, int32_t dtype, int64_t M, int32_t Kd, int32_t form);
int kasf_op_mlp_bwd_rows(int32_t dtype, const void* x, const void* g, const float* ln_g, const float* ln_b, const void* w1, const float* b1,
                         const void* w2t_scaled, const void* w1t, void* hbuf, void* dzbuf, void* g_in, float* dgamma, float* dbeta, int64_t M, float* scratch,
                         int64_t scratch_floats, void* stream);
int kasf_op_dgrad_lnbwd_rows(int32_t dtype, const void* dy, int32_t Kd, const void* wt, const void* dxn_add, const void* x, const float* gamma,
                             const void* resid, void* out, int32_t accumulate, float* dgamma, float* dbeta, int64_t M, void* xn_out, const float* beta,
                             float* scratch, int64_t scratch_floats, void* stream);
int kasf_op_gcn_bwd_rows(int32_t dtype, const void* g, const void* xn, const void* y, const float* coef, const uint32_t* mask, const float* ls1, void* r, void* duv,
                         float* dls1, float* d_bn_w, float* d_bn_b, void* bstats, int32_t batch, int32_t n_frames, int32_t mode, int32_t training, float* scratch,
                         int64_t scratch_floats, void* stream);
/* bf16 only: kasf_op_mlp_bwd_fused with fc2 finished as a backward stage finishes it.  w2 [128,512] is the fp32 master of fc2 (w2t_scaled stays the bf16 copy of
 * (ls2 . W2)^T), b2 and ls2 [128] fp32.  With G = g^T H and c = colsum(g):
 *   dw1, db1, dgamma, dbeta are ACCUMULATED into, as there;
 *   dw2 [128,512] += ls2[n] G[n][:]  (the SCALED gradient);   dls2 [128] += <w2[n], G[n]> + b2 . c;
 *   the gsum slot is ASSIGNED db2 = ls2 . c  (what was there before is lost: it is the bias gradient's slot, written once per step).
 * This form has no atomics fallback: without the rows the finish that scales db2 and adds the b2 term never runs.  So a scratch that is NULL or below
 * kasf_op_sink_scratch_floats(KASF_SINK_MLP_BWD_FUSED_FC2, ...) is error 2 before any launch, never error 6 after one.  M <= 0: returns 0 after the checks. */
int kasf_op_mlp_bwd_fused_fc2(const void* x, const void* xn, const void* g, const float* ln_g, const void* w1, const float* b1, const void* w2t_scaled,
                              const void* w1t, void* dapart, float* partial, float* dw1, float* dw2, float* db1, float* gsum, void* g_in, float* dgamma,
                              float* dbeta, int64_t M, const float* w2, const float* b2, const float* ls2, float* dls2, float* scratch, int64_t scratch_floats,
                              void* stream);
/* ---- the prologue, gate, head and embedding kernels on their own (ADDED under ABI 12: additive, kasf_version() stays 12; a library without them fails to load on
 * the missing symbol).  Thin entries over the launches kasf_forward / kasf_backward make (k_misc.hip, k_reduce.hip), for unit tests against fp64 math.
 * Tensors of the model dtype are void*, everything else fp32.  frames = clips * n_frames, M = frames * 17 tokens in [clip][frame][joint] order.
 * scratch / scratch_floats (embed_bwd, refusion_bwd, gate_bwd, head_bwd): device floats, 16-byte aligned, at least kasf_op_misc_scratch_floats(op, n).  Given: every
 * workgroup stores its sums as one row of it and the entry finishes them in a fixed order on `stream` (what a backward stage does: bit-reproducible).  NULL: fp32
 * atomics.  Scratch that is too small: the launch falls back to the atomics (results still complete) and the entry returns error 6.
 * Gradients of parameters (dw, db, dpos, dls, grads) are ACCUMULATED into; everything else is written.
 * Error 2, before any device is touched: a required pointer that is null, frames < 1 or frames * 17 * 384 >= 2^31, M < 1 or M * 384 >= 2^31, scratch with
 * scratch_floats < 1 or misaligned, n of kasf_op_add not a multiple of 8 in [8, 2^40), (N, K) of kasf_op_finalize_ls other than (128, 128) / (128, 512).  Error 3: bad
 * dtype.  Error 4: a layout-only model where the entry needs the device tables (prologue_fwd, refusion_bwd). */
#define KASF_MISC_EMBED_BWD 0
#define KASF_MISC_REFUSION_BWD 1
#define KASF_MISC_GATE_BWD 2
#define KASF_MISC_HEAD_BWD 3
/* floats of scratch the op asks for at n = frames (embed, refusion) or M (gate, head); -2 with kasf_last_error() set for an unknown op or n < 1.  Needs no device. */
int64_t kasf_op_misc_scratch_floats(int32_t op, int64_t n);
/* x [frames,17,3] -> bone3 [frames,17,3] (direction x, y, length per bone, zero length -> 1; row 16 = mean of the 16), limb3 [frames,17,3] (the 51 limb MLPs on the raw
 * joints), xj / xb / xl [frames*17,128] model dtype = Linear(3,128)(x / bone3 / limb3) + position embedding.  params: the flat fp32 parameter array of `model`. */
int kasf_op_prologue_fwd(const kasf_model* model, const float* params, const float* x, void* xj, void* xb, void* xl, float* bone3, float* limb3, int64_t frames,
                         void* stream);
/* backward of one embedding: g [frames*17,128] model dtype, in3 [frames*17,3], w [128,3] -> dw [128,3], db [128], dpos [17,128] accumulated; din3 [frames*17,3] = g . w
 * written when not NULL. */
int kasf_op_embed_bwd(int32_t dtype, const void* g, const float* in3, const float* w, float* dw, float* db, float* dpos, float* din3, int64_t frames,
                      float* scratch, int64_t scratch_floats, void* stream);
/* backward of the 51 limb MLPs: x [frames,17,3] raw joints, dlimb3 [frames,17,3] -> the 204 limb-MLP tensors of grads (flat, laid out as params) accumulated; nothing
 * else of grads is touched. */
int kasf_op_refusion_bwd(const kasf_model* model, const float* params, const float* x, const float* dlimb3, float* grads, int64_t frames, float* scratch,
                         int64_t scratch_floats, void* stream);
/* backward of the prologue with respect to the keypoints (ADDED under ABI 12 as well; k_input_grad.hip, the launch kasf_backward makes under KASF_FLAG_INPUT_GRAD):
 * x [frames,17,3] raw joints; dx_joint3, dbone3, dlimb3 [frames,17,3] = din3 of the joints / bone / limb kasf_op_embed_bwd, any of them NULL = zero; all fp32
 * whatever the model dtype.  dx [frames,17,3] is WRITTEN:  dx = dx_joint3 + (bone decomposition)^T dbone3 + (the 51 limb MLPs' input gradients) dlimb3, where a
 * zero-length bone, whose length the forward replaced by the constant 1, passes its direction gradient through and its length gradient nowhere.  Every element is
 * summed in one fixed order (joints, then its bones by index, then the limb-MLP inputs that read it by group and slot): no atomics, the same bits from run to run,
 * and a frame's dx does not depend on the other frames of the call.  dx must not overlap an input.
 * Error 2, before any device is touched: model, params, x or dx null, frames < 1 or frames * 17 * 384 >= 2^31.  Error 4: a layout-only model. */
int kasf_op_input_grad(const kasf_model* model, const float* params, const float* x, const float* dx_joint3, const float* dbone3, const float* dlimb3,
                       float* dx, int64_t frames, void* stream);
/* alpha = softmax(cat(xa, xg, xb) w^T + bias) (w [3,384], bias [3]; adaptive == 0: 1/3 each), out = sum_k alpha_k x_k.  alpha [M,4] fp32 (slot 3 unused, not
 * written) or NULL. */
int kasf_op_gate_fwd(int32_t dtype, const void* xa, const void* xg, const void* xb, const float* w, const float* bias, void* out, float* alpha, int64_t M,
                     int32_t adaptive, void* stream);
/* gradients of the above for g (+ g1 + g2 when not NULL) = d/d(out), alpha as the forward stored it (16-byte aligned): ga / gg / gb [M,128] written; dw [3,384], db [3]
 * accumulated (adaptive == 0: untouched, may be NULL). */
int kasf_op_gate_bwd(int32_t dtype, const void* g, const void* g1, const void* g2, const void* xa, const void* xg, const void* xb, const float* w,
                     const float* alpha, void* ga, void* gg, void* gb, float* dw, float* db, int64_t M, int32_t adaptive, float* scratch,
                     int64_t scratch_floats, void* stream);
/* out [M,3] fp32 = rep w^T + bias; rep [M,512] model dtype = tanh features, w [3,512]. */
int kasf_op_head_fwd(int32_t dtype, const void* rep, const float* w, const float* bias, float* out, int64_t M, void* stream);
/* dy [M,3] fp32 -> dpre [M,512] model dtype = (dy w) (1 - rep^2) written; dw [3,512], db [3] accumulated. */
int kasf_op_head_bwd(int32_t dtype, const float* dy, const void* rep, const float* w, void* dpre, float* dw, float* db, int64_t M, float* scratch,
                     int64_t scratch_floats, void* stream);
/* return_rep backward: dpre [M,512] = drep (fp32) (1 - rep^2). */
int kasf_op_rep_bwd(int32_t dtype, const float* drep, const void* rep, void* dpre, int64_t M, void* stream);
/* layer-scale finish of a Linear [N,K] whose output is multiplied by ls [N]: in dw = unscaled g^T a, db = colsum(g); dls[n] += sum_k w[n][k] dw[n][k] + bias[n] db[n];
 * then dw[n][:] *= ls[n], db[n] *= ls[n] in place. */
int kasf_op_finalize_ls(float* dw, const float* w, const float* bias, const float* ls, float* db, float* dls, int32_t N, int32_t K, void* stream);
/* n elements of the model dtype: b == NULL: dst += a (c must be NULL too); otherwise dst = a + b (+ c when not NULL). */
int kasf_op_add(int32_t dtype, void* dst, const void* a, const void* b, const void* c, int64_t n, void* stream);
/* fp32 <-> model dtype */
int kasf_op_cast(int32_t dtype, const void* src, void* dst, int64_t n, int32_t to_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KASF_H_ */
