"""ctypes binding of libkasf_hip.so (C-ABI in include/kasf.h).

The library is built in-tree by ``kasportsformer_amd/csrc/Makefile`` (see ``__graft_entry__.build``).
There is NO fallback: if the shared object is missing or a symbol is absent the import raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KASF_LIB: another build of the same library (same-box A/B comparisons of kernel variants: tools/ab.sh); the default is the in-tree product build
LIB_PATH = os.environ.get("KASF_LIB") or os.path.join(_HERE, "libkasf_hip.so")

DTYPE_F32, DTYPE_BF16 = 0, 1
DTYPE_F16 = 2                          # KASF_DTYPE_F16: heatmap / detector input and crop output only, no model runs in it
GEOM_CENTER_SCALE, GEOM_BOX = 0, 1
LAYOUT_COCO, LAYOUT_H36M = 0, 1
DECODE_QUARTER, DECODE_DARK, DECODE_DARK_UDP = 0, 1, 2   # KASF_DECODE_*: the mode of kasf_heatmap_decode
ROWS_PERSONS, ROWS_TRACKS = 0, 1         # KASF_ROWS_*: row order of kasf_stream_track_front
DETECT_PREDICTION, DETECT_HEADS = 0, 1
DETECT_MAX_CANDIDATES = 4096           # KASF_DETECT_MAX_CANDIDATES
LETTERBOX_MAX_SIDE = 4096              # KASF_LETTERBOX_MAX_SIDE: out_w and out_h of kasf_letterbox_frames
YUV_NV12, YUV_I420 = 0, 1                # KASF_YUV_*: layout of kasf_yuv420_to_bgr
YUV_BT601, YUV_BT709 = 0, 1              # KASF_YUV_BT*: its matrix
DRAW_MAX_JOINTS, DRAW_MAX_SEGMENTS, DRAW_MAX_FILLS = 32, 32, 8      # kasf_draw_poses: J, S, R
DRAW_MAX_THICKNESS, DRAW_MAX_RADIUS = 64, 32
SORT_MAX = 64                          # KASF_SORT_MAX: slots and max_dets of kasf_sort_update
SORT_HEADER_BYTES = 64                 # KASF_SORT_HEADER_BYTES
MATCH_MAX_CAMERAS, MATCH_MAX_ROWS = 16, 64     # KASF_MATCH_MAX_CAMERAS, KASF_MATCH_MAX_ROWS: cameras, rows and max_groups of kasf_match_*
FLAG_TRAIN, FLAG_RETURN_REP, FLAG_KEEP = 1, 2, 4
FLAG_INPUT_GRAD = 8                    # KASF_FLAG_INPUT_GRAD: kasf_backward also leaves d/dx in the workspace entry "dx_input"
EVAL_COLS = 22
LOSS7_MAX_FRAMES = 360               # KASF_LOSS7_MAX_FRAMES: n_frames of kasf_loss7
MISC_EMBED_BWD, MISC_REFUSION_BWD, MISC_GATE_BWD, MISC_HEAD_BWD = 0, 1, 2, 3      # KASF_MISC_*: ops of kasf_op_misc_scratch_floats
SINK_MLP_BWD_FUSED_FC2, SINK_MLP_BWD_ROWS, SINK_DGRAD_LNBWD_ROWS, SINK_GCN_BWD_ROWS = 0, 1, 2, 3      # KASF_SINK_*: ops of kasf_op_sink_scratch_floats
SINK_FORM_RESID, SINK_FORM_DXN_ADD, SINK_FORM_ACCUMULATE, SINK_FORM_XN_OUT = 1, 2, 4, 8               # KASF_SINK_FORM_*
GCN_STAT_WORDS = 4 * 512 * 5    # KASF_GCN_STAT_WORDS: int64 words of one BatchNorm statistics buffer of kasf_op_gcn_fwd / kasf_op_gcn_bwd
OPT_CHUNK_MAX, OPT_MAX_CLASSES = 4096, 32      # KASF_OPT_CHUNK_MAX, KASF_OPT_MAX_CLASSES: kasf_adamw_segments / kasf_grad_norm
ABI_VERSION = 12        # kasf_version() of the library these prototypes describe (a stale in-tree .so is refused)


class KasfConfig(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("n_frames", C.c_int32), ("num_heads", C.c_int32), ("neighbour_num", C.c_int32),
                ("use_adaptive_fusion", C.c_int32), ("dtype", C.c_int32)]


class KasfOptChunk(C.Structure):         # one record of the chunk table of kasf_adamw_segments / kasf_grad_norm (numpy: optim.CHUNK_DTYPE)
    _fields_ = [("begin", C.c_int64), ("count", C.c_int32), ("cls", C.c_int32)]


class KasfAdamwClass(C.Structure):       # bc1 / bc2 are formed by the library from `step`
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("bc1", C.c_float),
                ("bc2", C.c_float), ("step", C.c_int32)]


class KasfOneEuroParams(C.Structure):     # kasf_one_euro_params: host values, passed by value into the launch
    _fields_ = [("dt", C.c_float), ("min_cutoff", C.c_float), ("d_cutoff", C.c_float), ("beta", C.c_float), ("min_score", C.c_float), ("max_hold", C.c_int32)]


class KasfPlaceParams(C.Structure):       # kasf_place_params: host values, passed by value into the launch
    _fields_ = [("min_score", C.c_float), ("weighted", C.c_int32), ("iterations", C.c_int32), ("delta", C.c_float), ("min_joints", C.c_int32)]


class KasfTriangulateParams(C.Structure):  # kasf_triangulate_params: host values, passed by value into the launch
    _fields_ = [("min_score", C.c_float), ("weighted", C.c_int32), ("iterations", C.c_int32), ("delta", C.c_float), ("min_views", C.c_int32),
                ("undistort_iterations", C.c_int32)]


class KasfMatchParams(C.Structure):        # kasf_match_params: host values, passed by value into the launch
    _fields_ = [("min_score", C.c_float), ("weighted", C.c_int32), ("cap", C.c_float), ("min_samples", C.c_int32), ("undistort_iterations", C.c_int32)]


class KasfRefineParams(C.Structure):      # kasf_refine_params: host values, passed by value into the launch; weights[k] = the weight at distance k frames
    _fields_ = [("min_score", C.c_float), ("max_gap", C.c_int32), ("radius", C.c_int32), ("weights", C.c_float * 33)]


class KasfError(RuntimeError):
    pass


_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
_pi64, _pi32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)

# name -> (restype, argtypes); every symbol declared in include/kasf.h
SIGNATURES = {
    "kasf_last_error": (C.c_char_p, []),
    "kasf_version": (_i32, []),
    "kasf_set_single_stream": (None, [_i32]),
    "kasf_set_fused_wgrad_min_tokens": (None, [_i64]),
    "kasf_get_fused_wgrad_min_tokens": (_i64, []),
    "kasf_get_single_stream": (_i32, []),
    "kasf_set_fused_attn_bwd": (None, [_i32]),
    "kasf_get_fused_attn_bwd": (_i32, []),
    "kasf_set_deterministic": (None, [_i32]),
    "kasf_get_deterministic": (_i32, []),
    "kasf_model_create": (_i32, [C.POINTER(KasfConfig), C.POINTER(_vp)]),
    "kasf_model_create_layout_only": (_i32, [C.POINTER(KasfConfig), C.POINTER(_vp)]),
    "kasf_model_destroy": (None, [_vp]),
    "kasf_model_status": (_i32, [_vp, _pi32]),
    "kasf_param_count": (_i64, [_vp]),
    "kasf_param_live_count": (_i64, [_vp]),
    "kasf_param_entries": (_i32, [_vp]),
    "kasf_param_entry": (_i32, [_vp, _i32, C.c_char_p, _i32, _pi64, _pi32, _pi64]),
    "kasf_buffer_count": (_i64, [_vp]),
    "kasf_buffer_entries": (_i32, [_vp]),
    "kasf_buffer_entry": (_i32, [_vp, _i32, C.c_char_p, _i32, _pi64, _pi32, _pi64]),
    "kasf_backward_stages": (_i32, [_vp]),
    "kasf_stage_grad_range": (_i32, [_vp, _i32, _pi64, _pi64]),
    "kasf_packed_bytes": (_i64, [_vp]),
    "kasf_pack_weights": (_i32, [_vp, _vp, _vp, _vp]),
    "kasf_workspace_bytes": (_i64, [_vp, _i32, _i32]),
    "kasf_forward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "kasf_backward": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "kasf_loss3": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _f32, _f32, _vp]),
    "kasf_loss7": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, C.POINTER(_f32), _f32, _vp]),
    "kasf_adamw_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _vp]),
    "kasf_adamw_segments": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, C.POINTER(KasfAdamwClass), _i32, _f32, _vp, _vp]),
    "kasf_grad_norm": (_i32, [_vp, _i64, _vp, _i64, _vp, _f32, _f32, _vp, _vp]),
    "kasf_gather_clips": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "kasf_joint_flip": (_i32, [_vp, _vp, _i64, _vp]),
    "kasf_tta_merge": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "kasf_eval_metrics": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kasf_lift_window_count": (_i64, [_i64, _i32, _i32]),
    "kasf_lift_windows": (_i32, [_vp, _i32, _i64, _f32, _f32, _i32, _i32, _vp, _i32, _vp, _vp]),
    "kasf_lift_stitch": (_i32, [_vp, _i32, _i32, _i64, _i32, _i32, _vp, _vp, _vp]),
    "kasf_lift_ragged_plan": (_i64, [_vp, _i32, _i32, _i32, _vp]),
    "kasf_lift_windows_ragged": (_i32, [_vp, _vp, _vp, _i32, _i64, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp]),
    "kasf_lift_stitch_ragged": (_i32, [_vp, _i32, _vp, _vp, _i32, _i64, _i64, _i32, _i32, _vp, _vp, _vp]),
    "kasf_stream_tables": (_i32, [_i32, _vp, _vp]),
    "kasf_stream_push": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "kasf_stream_windows": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "kasf_stream_emit": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "kasf_stream_track_front": (_i32, [_vp] * 5 + [_i32] * 5 + [_vp] * 6 + [_i32, _vp, _vp, _vp]),
    "kasf_stream_track_emit": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "kasf_one_euro_push": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(KasfOneEuroParams), _i64, _vp, _vp, _vp, _vp, _vp]),
    "kasf_one_euro_tracked": (_i32, [_vp] * 5 + [_i32] * 7 + [C.POINTER(KasfOneEuroParams), _i64] + [_vp] * 7),
    "kasf_one_euro_tracks": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, C.POINTER(KasfOneEuroParams), _vp, _vp]),
    "kasf_tracks_refine": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, C.POINTER(KasfRefineParams), _vp, _vp, _vp]),
    "kasf_bone_median": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "kasf_bone_apply": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp]),
    "kasf_bone_push": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "kasf_bone_tracked": (_i32, [_vp] * 5 + [_i32] * 6 + [_vp] * 6),
    "kasf_pose_place": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _i32, C.POINTER(KasfPlaceParams)] + [_vp] * 6),
    "kasf_keypoints_triangulate": (_i32, [_vp, _i32, _i64, _i32, _vp, _i32, C.POINTER(KasfTriangulateParams)] + [_vp] * 6),
    "kasf_keypoints_undistort": (_i32, [_vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp]),
    "kasf_match_workspace_bytes": (_i64, [_i32, _i32, _i64]),
    "kasf_match_pair_costs": (_i32, [_vp, _i32, _i32, _i64, _i32, _vp, C.POINTER(KasfMatchParams), _vp, _vp, _vp, _i64, _vp]),
    "kasf_match_groups": (_i32, [_vp, _vp, _i32, _i32, _f32, _i32] + [_vp] * 7),
    "kasf_coco_h36m": (_i32, [_vp, _i64, _vp, _vp]),
    "kasf_pose_world": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _vp, _vp]),
    "kasf_heatmap_keypoints": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _i32, C.c_double, _i32, _i32, _vp, _vp, _vp]),
    "kasf_heatmap_flip_keypoints": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _vp, _i32, _vp, _i32, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp]),
    "kasf_heatmap_decode": (_i32, [_vp, _vp, _i32, _i64, _i32, _i32, _vp, _i32, _vp, _i32, C.c_double, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "kasf_crop_persons": (_i32, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _i32, C.c_double, _i64, _vp, _i32, _i32, _i32, C.POINTER(_f32), _i32, _vp, _vp]),
    "kasf_letterbox_plan": (_i32, [_i32, _i32, _i32, _i32, _pi32, _pi32, _pi32, _pi32]),
    "kasf_letterbox_frames": (_i32, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "kasf_yuv420_to_bgr": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "kasf_draw_poses": (_i32, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _vp, _i32, _i32, _f32,
                              _vp, _i32, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _vp]),
    "kasf_bgr_to_nv12": (_i32, [_vp, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _vp]),
    "kasf_pose_panel": (_i32, [_vp, _i64, C.POINTER(_f32), _vp, _vp]),
    "kasf_detect_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "kasf_detect_boxes": (_i32, [_vp, _i32, _i32, _i32, _i32, _pi32, _i32, _i32, C.POINTER(_f32), _i32, _vp, _f32, _f32, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                 _i64, _vp]),
    "kasf_sort_state_bytes": (_i64, [_i32, _i32, _i32]),
    "kasf_sort_update": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _i32, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kasf_ws_entries": (_i32, [_vp, _i32, _i32]),
    "kasf_ws_entry": (_i32, [_vp, _i32, _i32, _i32, C.c_char_p, _i32, _pi64, _pi64, _pi32]),
    "kasf_op_linear": (_i32, [_i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp]),
    "kasf_op_linear_res": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "kasf_op_mlp_fwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "kasf_op_mlp_bwd": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "kasf_op_mlp_bwd_fused": (_i32, [_vp] * 17 + [_i64, _vp]),
    "kasf_op_wgrad": (_i32, [_i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "kasf_op_dgrad_lnbwd": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp]),
    "kasf_op_dgrad_wg": (_i32, [_vp, _i32] + [_vp] * 7 + [_i32] + [_vp] * 11 + [_i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "kasf_op_wgrad_jobs": (_i32, [_i32] + [_vp] * 5 + [_i32] + [_vp] * 4 + [_i64, _vp, _i64, _i32] + [_vp] * 6 + [_i32, _vp, _vp, _vp]),
    "kasf_op_attention_fwd": (_i32, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _vp]),
    "kasf_op_attention_bwd": (_i32, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "kasf_op_attention_fwd_heads": (_i32, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp]),
    "kasf_op_attention_bwd_heads": (_i32, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "kasf_op_attention_bwd_fused_do": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "kasf_op_attn_block_fwd": (_i32, [_i32] + [_vp] * 16 + [_i32, _i32, _i32, _vp]),
    "kasf_op_attn_block_bwd": (_i32, [_i32] + [_vp] * 30 + [_i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp]),
    "kasf_op_gcn_fwd": (_i32, [_i32] + [_vp] * 13 + [_i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "kasf_op_gcn_bwd": (_i32, [_i32] + [_vp] * 12 + [_i32, _i32, _i32, _i32, _vp]),
    "kasf_op_sink_scratch_floats": (_i64, [_i32, _i32, _i64, _i32, _i32]),
    "kasf_op_mlp_bwd_rows": (_i32, [_i32] + [_vp] * 13 + [_i64, _vp, _i64, _vp]),
    "kasf_op_mlp_bwd_fused_fc2": (_i32, [_vp] * 17 + [_i64] + [_vp] * 5 + [_i64, _vp]),
    "kasf_op_dgrad_lnbwd_rows": (_i32, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "kasf_op_gcn_bwd_rows": (_i32, [_i32] + [_vp] * 12 + [_i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "kasf_op_misc_scratch_floats": (_i64, [_i32, _i64]),
    "kasf_op_prologue_fwd": (_i32, [_vp] * 8 + [_i64, _vp]),
    "kasf_op_embed_bwd": (_i32, [_i32] + [_vp] * 7 + [_i64, _vp, _i64, _vp]),
    "kasf_op_refusion_bwd": (_i32, [_vp] * 5 + [_i64, _vp, _i64, _vp]),
    "kasf_op_input_grad": (_i32, [_vp] * 7 + [_i64, _vp]),
    "kasf_op_gate_fwd": (_i32, [_i32] + [_vp] * 7 + [_i64, _i32, _vp]),
    "kasf_op_gate_bwd": (_i32, [_i32] + [_vp] * 13 + [_i64, _i32, _vp, _i64, _vp]),
    "kasf_op_head_fwd": (_i32, [_i32] + [_vp] * 4 + [_i64, _vp]),
    "kasf_op_head_bwd": (_i32, [_i32] + [_vp] * 6 + [_i64, _vp, _i64, _vp]),
    "kasf_op_rep_bwd": (_i32, [_i32] + [_vp] * 3 + [_i64, _vp]),
    "kasf_op_finalize_ls": (_i32, [_vp] * 6 + [_i32, _i32, _vp]),
    "kasf_op_add": (_i32, [_i32] + [_vp] * 4 + [_i64, _vp]),
    "kasf_op_cast": (_i32, [_i32, _vp, _vp, _i64, _i32, _vp]),
}
_EXTRA = {}

_lib = None


def load():
    """Loads the shared library (once) and attaches prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KasfError(
            f"{LIB_PATH} is missing: build it with `make -C kasportsformer_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "kasportsformer_amd has no CPU or eager-PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in {**SIGNATURES, **_EXTRA}.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.kasf_version() != ABI_VERSION:
        raise KasfError(f"{LIB_PATH} is version {lib.kasf_version()}, the host code expects {ABI_VERSION}: rebuild it (make -C kasportsformer_amd/csrc)")
    _lib = lib
    return lib


def check(code: int):
    if code != 0:
        msg = load().kasf_last_error()
        raise KasfError(f"libkasf_hip error {code}: {msg.decode() if msg else ''}")


def _entries(count_fn, entry_fn, handle, *pre):
    out = []
    name = C.create_string_buffer(256)
    off, ndim, shape = C.c_int64(), C.c_int32(), (C.c_int64 * 4)()
    for i in range(count_fn(handle, *pre)):
        check(entry_fn(handle, *pre, i, name, 256, C.byref(off), C.byref(ndim), shape))
        out.append((name.value.decode(), off.value, tuple(shape[k] for k in range(ndim.value))))
    return out


def param_entries(handle):
    lib = load()
    return _entries(lib.kasf_param_entries, lib.kasf_param_entry, handle)


def buffer_entries(handle):
    lib = load()
    return _entries(lib.kasf_buffer_entries, lib.kasf_buffer_entry, handle)


def ws_entries(handle, batch, flags):
    lib = load()
    out = {}
    name = C.create_string_buffer(256)
    off, numel, kind = C.c_int64(), C.c_int64(), C.c_int32()
    for i in range(lib.kasf_ws_entries(handle, batch, flags)):
        check(lib.kasf_ws_entry(handle, batch, flags, i, name, 256, C.byref(off), C.byref(numel), C.byref(kind)))
        out[name.value.decode()] = (off.value, numel.value, kind.value)
    return out


def ws_last_entry(handle, batch, flags):
    """(name, byte offset, numel, kind) of the LAST workspace entry: two plan walks instead of the one per entry that ws_entries costs (a 26-layer plan has
    some 1,500 entries), for the hot path -- KASF_FLAG_INPUT_GRAD puts "dx_input" there."""
    lib = load()
    name = C.create_string_buffer(64)
    off, numel, kind = C.c_int64(), C.c_int64(), C.c_int32()
    check(lib.kasf_ws_entry(handle, batch, flags, lib.kasf_ws_entries(handle, batch, flags) - 1, name, 64, C.byref(off), C.byref(numel), C.byref(kind)))
    return name.value.decode(), off.value, numel.value, kind.value
