"""Every refusal of the C entry points in csrc/api_video.hip and csrc/api_ops.hip, as a table (tests/test_refusals_cpu.py replays it against
tests/golden/refusals.json; tests/golden/make_refusals_golden.py recorded that file).

An entry of ENTRIES is ``(name, baseline, cases, nullable)``:

  name       the exported function; its parameter names and types are read from include/kasf.h.
  baseline   parameter -> value of a call that passes every check.  A parameter that is not named is 0 when it is a scalar and a zeroed, 64-byte aligned
             host buffer of BUF_BYTES of its own when it is a pointer (``stream`` is NULL).  The baseline itself is never called: it would reach a launch.
  cases      ``(case id, overrides)`` in the order of the checks in the source, one per refusal statement; a third element names an earlier case whose message this
             one must repeat (two violations in one parameter).  An override is a scalar, ``None`` (a null
             pointer), a ctypes object (a host buffer with that content), ``BUF`` (a fresh buffer), ``OFF(k)`` (a fresh buffer's address + k bytes) or
             ``SAME(p)`` (the pointer that parameter p gets).
  nullable   the pointer parameters that may be NULL in the baseline call (ALL: the entry checks no pointer).

``cases_of`` adds to these, per entry: one ``null:<p>`` case per other pointer parameter with that pointer alone NULL; ``all_wrong``, every pointer NULL and every
scalar -1 (it pins which check comes first); and ``pair:<a>+<b>`` for every two consecutive cases whose overrides do not touch the same parameter: both
violations at once, which must give the message of <a> (``replay`` checks that), since the order of the checks is what a refactor can change unnoticed.
"""
import ctypes as C
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KASF_LIB") or os.path.join(ROOT, "kasportsformer_amd", "libkasf_hip.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "refusals.json")
BUF_BYTES = 4096
ALL = "*"
INT64_MAX = 2 ** 63 - 1


class _Marker:
    def __init__(self, kind, arg=None):
        self.kind, self.arg = kind, arg


BUF = _Marker("buf")


def OFF(k):
    return _Marker("off", k)


def SAME(p):
    return _Marker("same", p)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def i64(*v):
    return (C.c_int64 * len(v))(*v)


def f32(*v):
    return (C.c_float * len(v))(*v)


class OneEuro(C.Structure):      # kasf_one_euro_params
    _fields_ = [("dt", C.c_float), ("min_cutoff", C.c_float), ("d_cutoff", C.c_float), ("beta", C.c_float), ("min_score", C.c_float), ("max_hold", C.c_int32)]


def euro(**kw):
    return OneEuro(**{**dict(dt=1 / 30, min_cutoff=1.0, d_cutoff=1.0, beta=0.0, min_score=0.0, max_hold=0), **kw})


class AdamwClass(C.Structure):   # KasfAdamwClass
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("bc1", C.c_float),
                ("bc2", C.c_float), ("step", C.c_int32)]


_KEEP = []                       # buffers that a pointer array points into


def ptrs(*bufs):
    """A host array of pointers (kasf_detect_boxes' src): to fresh buffers, or NULL where None is given."""
    out = (C.c_void_p * len(bufs))()
    for k, b in enumerate(bufs):
        if b is not None:
            _KEEP.append(C.create_string_buffer(BUF_BYTES))
            out[k] = C.addressof(_KEEP[-1])
    return out


def aptrs(*offsets):
    """A host array of pointers (kasf_op_wgrad_jobs' per-job arrays): entry k points `offsets[k]` bytes behind a 64-byte boundary of a fresh buffer, or is NULL for None."""
    out = (C.c_void_p * len(offsets))()
    for k, off in enumerate(offsets):
        if off is not None:
            _KEEP.append(C.create_string_buffer(BUF_BYTES + 64))
            out[k] = (C.addressof(_KEEP[-1]) + 63) // 64 * 64 + off
    return out


COCO_PAIRS = (0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15)
NOT_INVOLUTION = (1, 2, 0) + tuple(range(3, 17))
_PARTNER = [("partner_range", dict(partner=i32(17, *COCO_PAIRS[1:]))), ("partner_neg", dict(partner=i32(-1, *COCO_PAIRS[1:]))),
            ("partner_both", dict(partner=i32(17, 2, 0, *range(3, 17))), "partner_range"), ("involution", dict(partner=i32(*NOT_INVOLUTION)))]
NAN, INF = math.nan, math.inf

# what kasf_lift_windows ... kasf_stream_emit share
_LIFT = [("T", dict(T=0)), ("stride", dict(stride=4)), ("n", dict(n=-1))]
_RAGGED = [("T", dict(T=0)), ("stride", dict(stride=4)), ("negative", dict(tracks=-1)), ("plan", dict(frames=0))]
_STREAM = [("T", dict(T=0)), ("K", dict(K=3))]          # the third check of stream_error is null:slots
_TRACKED = [("streams", dict(streams=0)), ("track_slots", dict(track_slots=65)), ("R", dict(R=0)), ("rows_mode", dict(rows_mode=2)),
            ("bits_R", dict(streams=2 ** 30, R=4)), ("bits_slots", dict(streams=2 ** 30, track_slots=64))]
_EURO = [("J", dict(J=0)), ("C", dict(C=5)), ("hz", dict(params=euro(dt=0.0))), ("hz_nan", dict(params=euro(d_cutoff=NAN))), ("beta", dict(params=euro(beta=-1.0))),
         ("min_score", dict(params=euro(min_score=INF))), ("max_hold", dict(params=euro(max_hold=-1)))]
_HEATMAP = [("n", dict(n=-1)), ("HW", dict(H=0)), ("HW_big", dict(H=4097, W=4097)), ("dtype", dict(dtype=3)), ("geom_kind", dict(geom_kind=2)),
            ("out_layout", dict(out_layout=2)), ("aspect", dict(geom_kind=1, aspect=0.0)), ("h36m_scratch", dict(out_layout=1, coco_scratch=None))]
_HEATMAP_BASE = dict(dtype=0, n=1, H=4, W=4, geom_kind=0, aspect=0.75, out_layout=0)
_FRAMES_BASE = dict(n_frames=1, Hf=8, Wf=8, row_stride=24, frame_stride=192)
_NV12_OUT = dict(y_row_stride=8, uv_row_stride=8, y_frame_stride=64, uv_frame_stride=32, matrix=0)
_DETECT_SHAPE = [("batch", dict(batch=-1)), ("max_candidates", dict(max_candidates=0))]
_SORT_SHAPE = [("streams", dict(streams=-1)), ("slots", dict(slots=0)), ("max_dets", dict(max_dets=0))]
_SORT_BASE = dict(streams=1, slots=4, max_dets=4)
_DT = [("dtype", dict(dtype=2))]
_GCN = _DT + [("mode", dict(mode=2)), ("n_frames", dict(n_frames=3)), ("batch", dict(batch=0)), ("batch_big", dict(batch=2 ** 24, n_frames=256))]
_SCRATCH = [("scratch_floats", dict(scratch_floats=0)), ("scratch_align", dict(scratch=OFF(4)))]

# kasf_op_dgrad_wg: the eight arguments of its PROJ form, absent and present, and the bytes of 256 bf16 tiles of 128 x 128
_NO_PROJ = dict(proj_o=None, proj_w=None, proj_b=None, proj_ls=None, dproj_w=None, dproj_b=None, dproj_ls=None, proj_part=None)
_WG_TILES = 256 * 128 * 128 * 2
_PROJ = dict({p: BUF for p in _NO_PROJ}, proj_part_bytes=_WG_TILES + 256 * 128 * 4)

# kasf_op_wgrad_jobs: one job of N = 128 without a fin job (its host arrays hold three entries, so that a case may raise njobs), the fin job's and the ext job's
# arguments, and one reduction
_JOBS_BASE = dict(njobs=1, g=aptrs(0, 0, 0), x=aptrs(0, 0, 0), N=i32(128, 128, 128), dw=aptrs(0, 0, 0), dbias=aptrs(None, None, None), fin_job=-1, M=1,
                  partial_floats=128 * 128, nred=0, fin_w=None, fin_bias=None, fin_ls=None, dls=None, red_part=None, red_out=None, red_nparts=None, red_elems=None,
                  ext_part=None, ext_brow=None, ext_nparts=0, ext_dw=None, ext_db=None)
_JOBS_FIN = dict(fin_job=0, dbias=aptrs(0, None, None), fin_w=BUF, fin_bias=BUF, fin_ls=BUF, dls=BUF)
_JOBS_EXT = dict(ext_part=BUF, ext_brow=BUF, ext_nparts=1, ext_dw=BUF, ext_db=BUF)
_JOBS_RED = dict(nred=1, red_part=aptrs(0), red_out=aptrs(0), red_nparts=i32(1), red_elems=i32(128))

# the attention entries: what kasf_op_attention_* check alike behind their dtype (api_ops.hip, attn_core_check), and the block forward's absent / present operands
_ATTN_BASE = dict(dtype=0, batch=1, n_frames=4, ldq=128, ldkv=128)
_ATTN_BWD_BASE = dict(_ATTN_BASE, lddq=128, lddkv=128)
_ATTN_SHAPE = [("mode", dict(mode=2)), ("batch", dict(batch=-1)), ("n_frames", dict(n_frames=0)), ("big", dict(batch=2 ** 20, n_frames=2 ** 10)),
               ("big_ld", dict(batch=2 ** 10, n_frames=2 ** 5, ldkv=4096), "big")]
_ATTN_LD = [("ldq", dict(ldq=120)), ("ldq_8", dict(ldq=132)), ("ldkv", dict(ldkv=64)), ("ldkv_8", dict(ldkv=388)), ("lddq", dict(lddq=0)), ("lddq_8", dict(lddq=129)),
            ("lddkv", dict(lddkv=-128)), ("lddkv_8", dict(lddkv=260))]
_ATTN_ALIGN = [("align", dict(q=OFF(8))), ("align_o", dict(o=OFF(4)), "align")]
_ATTN_FUSED_BASE = {k: v for k, v in _ATTN_BWD_BASE.items() if k != "dtype"}
_BLK_BASE = dict(bone=0, batch=1, n_frames=4, mode=0, x_limb=None, lnl_g=None, lnl_b=None, wkv=None, q_save=None, kv_save=None, o_save=None, lse_save=None)
_BLK_BONE = dict(bone=1, x_limb=BUF, lnl_g=BUF, lnl_b=BUF, wkv=BUF)
# kasf_op_attn_block_bwd: one spatial frame of the self-attention form (68 tokens: one split), the eleven arguments of the bone form absent
_BWD_BONE_ARGS = ("x_limb", "lnl_g", "lnl_b", "wkv", "wq_t", "out_limb", "dkv", "xn_b", "dgamma_l", "dbeta_l", "dw_kv")
_BWD_BASE = dict({p: None for p in _BWD_BONE_ARGS}, bone=0, batch=1, n_frames=4, mode=0, partial_floats=384 * 128, proj_part_bytes=_WG_TILES + 256 * 128 * 4,
                 scratch_floats=256)

ENTRIES = [
    # ---- api_ops.hip: loss, optimizer, data, eval ----
    ("kasf_loss3", dict(losses_floats=12, batch=2, n_frames=3), [("shape", dict(batch=0)), ("shape_T", dict(n_frames=0)), ("losses", dict(losses_floats=11))], ()),
    ("kasf_loss7", dict(losses_floats=24, batch=2, n_frames=3),
     [("shape", dict(batch=0)), ("shape_T", dict(n_frames=0)), ("max_frames", dict(n_frames=361)), ("losses", dict(losses_floats=23))], ()),
    ("kasf_adamw_step", dict(n=8, step_index=1), [("n", dict(n=6)), ("step", dict(step_index=0))], ()),
    ("kasf_adamw_segments", dict(n=8, n_chunks=1, n_classes=1, classes=AdamwClass(step=1), grad_scale=1.0),
     [("align", dict(params=OFF(4))), ("align_sq", dict(exp_avg_sq=OFF(8))), ("count", dict(n=-1)), ("count_chunks", dict(n_chunks=-1)),
      ("n_classes", dict(n_classes=0)), ("n_classes_big", dict(n_classes=33)), ("class_step", dict(classes=AdamwClass(step=0)))], ("clip",)),
    ("kasf_grad_norm", dict(n=8, n_chunks=1), [("align", dict(grads=OFF(4))), ("count", dict(n=-1)), ("count_chunks", dict(n_chunks=-1))], ()),
    ("kasf_gather_clips", dict(n_clips=1, batch=1, n_frames=1), [("empty", dict(n_clips=0)), ("empty_T", dict(n_frames=0))], ("y_all", "flip")),
    ("kasf_joint_flip", dict(rows=1), [("aliased", dict(dst=SAME("src")))], ()),
    ("kasf_tta_merge", dict(rows=1), [], ("pred_of_flipped",)),
    ("kasf_eval_metrics", dict(batch=1, n_frames=3, n_actions=1), [("n_frames", dict(n_frames=2)), ("n_frames_big", dict(n_frames=257))], ()),
    # ---- api_video.hip: lift ----
    ("kasf_lift_window_count", dict(n=5, T=3, stride=1), [_LIFT[0], ("T_big", dict(T=257)), _LIFT[1], ("stride_0", dict(stride=0)), _LIFT[2]], ()),
    ("kasf_lift_windows", dict(persons=1, n=5, width=1.0, height=1.0, T=3, stride=1),
     _LIFT + [("persons", dict(persons=-1)), ("size", dict(width=0.0)), ("size_nan", dict(height=NAN)), ("table", dict(n=2, resample=None))], ("resample",)),
    ("kasf_lift_stitch", dict(persons=1, n=5, T=3, stride=1), _LIFT + [("persons", dict(persons=-1)), ("table", dict(n=2, first_pos=None))], ("first_pos",)),
    ("kasf_lift_ragged_plan", dict(lengths=i64(5), tracks=1, T=3, stride=1),
     [("T", dict(T=0)), ("stride", dict(stride=4)), ("tracks", dict(tracks=-1)), ("length", dict(lengths=i64(-1))),
      ("overflow", dict(lengths=i64(INT64_MAX, INT64_MAX), tracks=2, T=1))], ()),
    ("kasf_lift_windows_ragged", dict(tracks=1, frames=5, windows=3, T=3, stride=1), _RAGGED + [("plan_more", dict(windows=6)), ("plan_none", dict(tracks=0))], ()),
    ("kasf_lift_stitch_ragged", dict(tracks=1, frames=5, windows=3, T=3, stride=1), _RAGGED, ()),
    # ---- stream, stream_track, one_euro ----
    ("kasf_stream_tables", dict(T=2), [("T", dict(T=0)), ("T_big", dict(T=257))], ()),
    ("kasf_stream_push", dict(K=1, S=2, T=3), _STREAM + [("S", dict(S=-1)), ("K_neg", dict(K=-1))], ()),
    ("kasf_stream_windows", dict(K=1, S=2, T=3), _STREAM, ()),
    ("kasf_stream_emit", dict(K=1, S=2, T=3, back=0, n_out=1),
     _STREAM + [("back", dict(back=3)), ("back_neg", dict(back=-1)), ("n_out", dict(n_out=4)), ("n_out_neg", dict(n_out=-1))], ()),
    ("kasf_stream_track_front", dict(streams=1, track_slots=2, rows_mode=0, R=1, T=3), [("T", dict(T=0)), ("T_big", dict(T=257))] + _TRACKED, ()),
    ("kasf_stream_track_emit", dict(n_rows=1, T=3, back=0), [("T", dict(T=0)), ("back", dict(back=3)), ("n_rows", dict(n_rows=-1))], ()),
    ("kasf_one_euro_push", dict(K=1, S=2, J=17, C=2, params=euro(), tick=0), _EURO + [("K", dict(K=3)), ("tick", dict(tick=-1))], ()),
    ("kasf_one_euro_tracked", dict(streams=1, track_slots=2, rows_mode=0, R=1, J=17, C=2, params=euro(), tick=0), _EURO + _TRACKED + [("tick", dict(tick=-1))],
     ("row_slot",)),
    ("kasf_one_euro_tracks", dict(N=1, P=1, J=17, C=2, params=euro()), _EURO + [("P", dict(P=-1)), ("N", dict(N=-1))], ()),
    # ---- coco and world, heatmap ----
    ("kasf_coco_h36m", dict(frames=1), [("frames", dict(frames=-1))], ()),
    ("kasf_pose_world", dict(frames=1), [("frames", dict(frames=-1))], ("trans3",)),
    ("kasf_heatmap_keypoints", _HEATMAP_BASE, _HEATMAP, ("coco_scratch",)),
    ("kasf_heatmap_flip_keypoints", dict(_HEATMAP_BASE, partner=i32(*COCO_PAIRS)),
     _HEATMAP[:7] + _PARTNER + [_HEATMAP[7], ("overlap", dict(merged_out=SAME("hm"))),
                     ("overlap_flipped", dict(merged_out=SAME("hm_flipped")))], ("partner", "coco_scratch", "merged_out")),
    ("kasf_heatmap_decode", dict(_HEATMAP_BASE, partner=i32(*COCO_PAIRS), mode=0, K=1),
     _HEATMAP[:7] + [("mode", dict(mode=3)), ("K", dict(K=2)), ("K_big", dict(K=19)), ("weights", dict(mode=1, weights=None)), ("udp", dict(udp=1, H=1)),
                     *_PARTNER,
                     ("involution_no_flip", dict(partner=i32(*NOT_INVOLUTION), hm_flipped=None, merged_out=None)), _HEATMAP[7],
                     ("merged_alone", dict(hm_flipped=None)), ("overlap", dict(merged_out=SAME("hm"))), ("overlap_flipped", dict(merged_out=SAME("hm_flipped")))],
     ("partner", "weights", "coco_scratch", "merged_out")),
    # ---- crop, letterbox, yuv, draw ----
    ("kasf_crop_persons", dict(_FRAMES_BASE, geom_kind=0, aspect=0.75, n=1, out_dtype=0, out_w=4, out_h=4, mean_std=f32(0, 0, 0, 1, 1, 1)),
     [("n", dict(n=-1)), ("out", dict(out_w=0)), ("out_big", dict(out_h=32768)), ("frame", dict(Hf=0)), ("frame_big", dict(Wf=32768, row_stride=3 * 32768)),
      ("n_frames", dict(n_frames=0)), ("row_stride", dict(row_stride=23)), ("frame_stride", dict(n_frames=2, frame_stride=-1)), ("out_dtype", dict(out_dtype=3)),
      ("geom_kind", dict(geom_kind=2)), ("aspect", dict(geom_kind=1, aspect=0.0)), ("std_zero", dict(mean_std=f32(0, 0, 0, 1, 0, 1))),
      ("std_inf", dict(mean_std=f32(0, 0, 0, 1, 1, INF))), ("frame_index", dict(n_frames=2, frame_index=None))], ("frame_index", "center_scale_out")),
    ("kasf_letterbox_plan", dict(Wf=8, Hf=8, out_w=4, out_h=4),
     [("frame", dict(Hf=0)), ("frame_big", dict(Wf=32768)), ("out", dict(out_w=0)), ("out_big", dict(out_h=4097)), ("elongated", dict(Wf=32767, Hf=1))], ()),
    ("kasf_letterbox_frames", dict(_FRAMES_BASE, out_dtype=0, out_w=4, out_h=4, pad_value=128),
     [("n_frames", dict(n_frames=-1)), ("frame", dict(Hf=0)), ("out", dict(out_w=0)), ("elongated", dict(Wf=32767, Hf=1, row_stride=3 * 32767)),
      ("row_stride", dict(row_stride=23)), ("frame_stride", dict(frame_stride=-1)), ("plane", dict(n_frames=2, frame_stride=191)), ("out_dtype", dict(out_dtype=3)),
      ("pad_value", dict(pad_value=256)), ("pad_value_neg", dict(pad_value=-1))], ()),
    ("kasf_yuv420_to_bgr", dict(c1=None, layout=0, n_frames=1, Hf=8, Wf=8, y_row_stride=8, c_row_stride=8, y_frame_stride=64, c_frame_stride=32,
                                out_row_stride=24, out_frame_stride=192, matrix=0),
     [("n_frames", dict(n_frames=-1)), ("frame", dict(Hf=0)), ("layout", dict(layout=2)), ("matrix", dict(matrix=2)), ("luma", dict(y_row_stride=7)),
      ("chroma", dict(c_row_stride=7)), ("chroma_i420", dict(layout=1, c1=BUF, c_row_stride=3)), ("out_row", dict(out_row_stride=23)),
      ("stride_y", dict(y_frame_stride=-1)), ("stride_c", dict(c_frame_stride=-1)), ("stride_out", dict(out_frame_stride=-1)),
      ("plane_y", dict(n_frames=2, y_frame_stride=63)), ("plane_c", dict(n_frames=2, c_frame_stride=31)), ("plane_out", dict(n_frames=2, out_frame_stride=191)),
      ("c1_nv12", dict(c1=BUF)), ("c1_i420", dict(layout=1, c1=None))], ("c1",)),
    ("kasf_draw_poses", dict(_FRAMES_BASE, **_NV12_OUT, P=1, J=17, C=2, S=1, thickness=1, out_row_stride=24, out_frame_stride=192),
     [("n_frames", dict(n_frames=-1)), ("frame", dict(Hf=0)), ("matrix", dict(matrix=2)), ("no_output", dict(out_bgr=None, out_y=None, out_uv=None)),
      ("half_surface", dict(out_uv=None)), ("row_stride", dict(row_stride=23)), ("frame_stride", dict(frame_stride=-1)), ("plane", dict(n_frames=2, frame_stride=191)),
      ("out_row", dict(out_row_stride=23)), ("out_stride", dict(out_frame_stride=-1)), ("out_plane", dict(n_frames=2, out_frame_stride=191)),
      ("luma", dict(y_row_stride=7)), ("chroma", dict(uv_row_stride=7)), ("stride_y", dict(y_frame_stride=-1)), ("stride_uv", dict(uv_frame_stride=-1)),
      ("plane_y", dict(n_frames=2, y_frame_stride=63)), ("plane_uv", dict(n_frames=2, uv_frame_stride=31)), ("P", dict(P=-1)), ("S", dict(S=33)),
      ("J", dict(J=0)), ("C", dict(C=4)), ("thickness", dict(thickness=0)), ("dot_radius", dict(dot_radius=33)), ("R", dict(R=9)),
      ("fills", dict(R=1, fills=None))], ("valid", "fills", "out_bgr")),
    ("kasf_bgr_to_nv12", dict(_FRAMES_BASE, **_NV12_OUT),
     [("n_frames", dict(n_frames=-1)), ("frame", dict(Hf=0)), ("matrix", dict(matrix=2)), ("row_stride", dict(row_stride=23)),
      ("frame_stride", dict(frame_stride=-1)), ("plane", dict(n_frames=2, frame_stride=191)), ("luma", dict(y_row_stride=7)), ("chroma", dict(uv_row_stride=7)),
      ("stride_y", dict(y_frame_stride=-1)), ("plane_uv", dict(n_frames=2, uv_frame_stride=31))], ()),
    ("kasf_pose_panel", dict(n=1), [("n", dict(n=-1)), ("n_big", dict(n=2 ** 40 + 1)), ("view", dict(view=f32(0, 0, 0, 0, 0, 0, 0, NAN)))], ()),
    # ---- detect, sort ----
    ("kasf_detect_workspace_bytes", dict(batch=1, n_per_image=10, max_candidates=16),
     [_DETECT_SHAPE[0], ("n_per_image", dict(n_per_image=0)), ("n_per_image_big", dict(n_per_image=2 ** 24 + 1)), _DETECT_SHAPE[1]], ()),
    ("kasf_detect_boxes", dict(src=ptrs(BUF), n_src=1, form=1, dtype=0, batch=1, grid=i32(13), A=3, C=80, inp_dim=416, confidence=0.5, nms=0.4, class_id=0,
                               max_candidates=16, max_boxes=4, workspace_bytes=2 ** 40),
     [("form", dict(form=2)), ("dtype", dict(dtype=3)), ("n_src", dict(n_src=0)), ("n_src_prediction", dict(form=0, n_src=2, src=ptrs(BUF, BUF), grid=i32(13, 26))),
      ("C", dict(C=0)), ("class_id", dict(class_id=80)), ("inp_dim", dict(inp_dim=0)), ("A", dict(A=9)), ("grid", dict(grid=i32(0))),
      ("grid_divide", dict(grid=i32(15))), _DETECT_SHAPE[0], ("candidates", dict(form=0, grid=i32(0))), _DETECT_SHAPE[1], ("max_boxes", dict(max_boxes=17)),
      ("finite", dict(confidence=NAN)), ("src_k", dict(src=ptrs(None))), ("workspace_align", dict(workspace=OFF(4))), ("workspace_bytes", dict(workspace_bytes=0))],
     ()),
    ("kasf_sort_state_bytes", _SORT_BASE, [_SORT_SHAPE[0], ("streams_big", dict(streams=65536)), _SORT_SHAPE[1], ("slots_big", dict(slots=65)), _SORT_SHAPE[2]], ()),
    ("kasf_sort_update", dict(_SORT_BASE, det_rows=1, det_stream_stride=4, det_row_stride=4, max_age=1, min_hits=1, iou_threshold=0.3, num_person=1),
     _SORT_SHAPE + [("det_rows", dict(det_rows=5)), ("det_row_stride", dict(det_row_stride=3)), ("det_stream_stride", dict(det_stream_stride=-1)),
                    ("max_age", dict(max_age=-1)), ("min_hits", dict(min_hits=-1)), ("iou", dict(iou_threshold=NAN)), ("num_person", dict(num_person=0)),
                    ("state_align", dict(state=OFF(4)))], ("det_count",)),
    # ---- api_ops.hip: the unit-test entries ----
    ("kasf_op_linear", dict(dtype=0, M=1, N=128), _DT + [("N", dict(N=100))], ALL),
    ("kasf_op_linear_res", dict(dtype=0, M=1), _DT, ()),
    ("kasf_op_mlp_fwd", dict(dtype=0, M=1), _DT, ALL),
    ("kasf_op_mlp_bwd", dict(dtype=0, M=1), _DT, ALL),
    ("kasf_op_mlp_bwd_fused", dict(M=1), [], ("ln_g", "w1", "b1", "w2t_scaled", "w1t", "dgamma", "dbeta")),
    ("kasf_op_sink_scratch_floats", dict(op=0, dtype=0, M=1, Kd=128),
     [("M", dict(M=0)), ("op", dict(op=4)), ("dtype", dict(op=1, dtype=2)), ("Kd", dict(op=2, Kd=100)), ("Kd_0", dict(op=2, Kd=0), "Kd")], ()),
    ("kasf_op_mlp_bwd_rows", dict(dtype=0, M=1, scratch_floats=256), _DT + _SCRATCH, ALL),
    # (M = 1: one token range of 512 floats and one streaming row of 384)
    ("kasf_op_mlp_bwd_fused_fc2", dict(M=1, scratch_floats=896), _SCRATCH + [("scratch_small", dict(scratch_floats=895))],
     ("ln_g", "w1", "b1", "w2t_scaled", "w1t", "dgamma", "dbeta")),
    ("kasf_op_wgrad", dict(dtype=0, N=128, K=128, M=1), _DT + [("N", dict(N=100)), ("K", dict(K=100)), ("ln_K", dict(K=256))], ALL),
    ("kasf_op_dgrad_lnbwd", dict(dtype=0, Kd=128, M=1), _DT + [("Kd", dict(Kd=100)), ("beta", dict(beta=None))], ALL),
    ("kasf_op_dgrad_lnbwd_rows", dict(dtype=0, Kd=128, M=1, scratch_floats=256), _DT + [("Kd", dict(Kd=100)), ("beta", dict(beta=None))] + _SCRATCH, ALL),
    ("kasf_op_dgrad_wg", dict(Kd=128, M=1, wpart_bytes=_WG_TILES, scratch_floats=256, dxn_add=None, dbias=None, **_NO_PROJ),
     [("proj_together", dict(proj_o=BUF)), ("form", dict(Kd=512)), ("form_resid", dict(resid=None), "form"), ("form_acc", dict(accumulate=1), "form"),
      ("form_uv", dict(Kd=256, dxn_add=BUF), "form"), ("form_proj", dict(Kd=384, **_PROJ), "form"), ("wpart_bytes", dict(wpart_bytes=_WG_TILES - 1)),
      ("proj_part_bytes", dict(_PROJ, proj_part_bytes=_WG_TILES + 256 * 128 * 4 - 1)), ("align", dict(wpart=OFF(4))),
      ("align_proj", dict(**{**_PROJ, "proj_part": OFF(8)}), "align")] + _SCRATCH + [("scratch_small", dict(M=33))],
     ("dxn_add", "resid", "dbias") + tuple(_NO_PROJ)),
    ("kasf_op_wgrad_jobs", _JOBS_BASE,
     [("njobs", dict(njobs=0)), ("njobs_big", dict(njobs=4), "njobs"), ("nred", dict(nred=3)), ("fin_job", dict(fin_job=1)), ("fin_job_neg", dict(fin_job=-2), "fin_job"),
      ("M_big", dict(M=2 ** 31)), ("null_red", dict(nred=1)), ("N", dict(N=i32(100, 128, 128))), ("N_640", dict(N=i32(640, 128, 128)), "N"),
      ("null_g_j", dict(g=aptrs(None)), "null_red"), ("null_red_k", dict(_JOBS_RED, red_part=aptrs(None)), "null_red"), ("align", dict(g=aptrs(8))),
      ("align_dbias", dict(dbias=aptrs(4)), "align"), ("align_partial", dict(partial=OFF(4)), "align"), ("align_ext", dict(ext_part=OFF(8)), "align"),
      ("dbias_job", dict(dbias=aptrs(0))), ("fin_vectors", dict(fin_job=0, dbias=aptrs(0))), ("fin_dbias", dict(_JOBS_FIN, dbias=aptrs(None)), "fin_vectors"),
      ("fin_N", dict(_JOBS_FIN, N=i32(256, 128, 128)), "fin_vectors"), ("ext_fin", dict(_JOBS_FIN, ext_part=BUF)), ("ext_njobs", dict(njobs=3, ext_part=BUF), "ext_fin"),
      ("ext_together", dict(ext_part=BUF)), ("ext_fin_vectors", dict(_JOBS_EXT), "ext_together"), ("ext_alone", dict(ext_nparts=1), "ext_together"),
      ("red_nparts", dict(_JOBS_RED, red_nparts=i32(0))), ("red_elems", dict(_JOBS_RED, red_elems=i32(100))), ("red_elems_0", dict(_JOBS_RED, red_elems=i32(0)), "red_elems"),
      ("partial_floats", dict(partial_floats=128 * 128 - 1)), ("partial_floats_fin", dict(_JOBS_FIN, partial_floats=128 * 128 + 127), "partial_floats")],
     ("fin_w", "fin_bias", "fin_ls", "dls", "red_part", "red_out", "red_nparts", "red_elems", "ext_part", "ext_brow", "ext_dw", "ext_db")),
    ("kasf_op_attention_fwd", _ATTN_BASE, _DT + _ATTN_SHAPE + _ATTN_LD[:4] + _ATTN_ALIGN, ()),
    ("kasf_op_attention_bwd", _ATTN_BWD_BASE, _DT + _ATTN_SHAPE + _ATTN_LD + [_ATTN_ALIGN[0], ("align_dv", dict(dv=OFF(4)), "align")], ()),
    ("kasf_op_attention_fwd_heads", dict(_ATTN_BASE, num_heads=8), _DT + _ATTN_SHAPE + _ATTN_LD[:4] + _ATTN_ALIGN, ()),
    ("kasf_op_attention_bwd_heads", dict(_ATTN_BWD_BASE, num_heads=8), _DT + _ATTN_SHAPE + _ATTN_LD + [_ATTN_ALIGN[0], ("align_dv", dict(dv=OFF(4)), "align")], ()),
    # (the first five cases are older than the shared checks: this entry refuses batch = 0, and its own messages come first)
    ("kasf_op_attention_bwd_fused_do", _ATTN_FUSED_BASE,
     [("form", dict(form=2)), ("batch", dict(batch=0)), ("batch_big", dict(batch=2 ** 20, n_frames=2 ** 10)), ("group", dict(mode=1, n_frames=97)),
      ("group_form1", dict(mode=1, n_frames=33, form=1)), ("mode", dict(mode=2)), ("big_ld", dict(batch=2 ** 10, n_frames=2 ** 5, lddkv=4096))] + _ATTN_LD
     + [("align", dict(g_mid=OFF(8))), ("align_lse", dict(lse=OFF(4)), "align")], ("o_saved", "lse")),
    ("kasf_op_attn_block_fwd", _BLK_BASE,
     [("bone", dict(bone=2)), ("mode", dict(mode=2)), ("batch", dict(batch=-1)), ("n_frames", dict(n_frames=0)), ("big", dict(batch=2 ** 20, n_frames=2 ** 10)),
      ("group", dict(mode=1, n_frames=97)), ("bone_operands", dict(bone=1)), ("bone_partial", dict(bone=1, x_limb=BUF, lnl_g=BUF, lnl_b=BUF), "bone_operands"),
      ("bone_extra", dict(x_limb=BUF), "bone_operands"), ("saves", dict(q_save=BUF)), ("saves_o", dict(q_save=None, o_save=BUF), "saves"),
      ("kv_save", dict(q_save=BUF, o_save=BUF, kv_save=BUF)), ("kv_save_bone", dict(_BLK_BONE, q_save=BUF, o_save=BUF), "kv_save"), ("lse_save", dict(lse_save=BUF)),
      ("alias", dict(out=SAME("x"))), ("align", dict(x=OFF(8))), ("align_out", dict(out=OFF(4)), "align"), ("align_save", dict(q_save=OFF(8), o_save=BUF), "align")],
     ("x_limb", "lnl_g", "lnl_b", "wkv", "q_save", "kv_save", "o_save", "lse_save")),
    ("kasf_op_attn_block_bwd", _BWD_BASE,
     [("bone", dict(bone=2)), ("mode", dict(mode=2)), ("batch", dict(batch=-1)), ("n_frames", dict(n_frames=0)), ("big", dict(batch=2 ** 20, n_frames=2 ** 10)),
      ("group", dict(mode=1, n_frames=33)), ("bone_operands", dict(bone=1)), ("bone_extra", dict(x_limb=BUF), "bone_operands"), ("alias", dict(out=SAME("x"))),
      ("align", dict(x=OFF(8))), ("align_dw", dict(dw_mix=OFF(4)), "align")] + _SCRATCH +
     [("proj_part_bytes", dict(proj_part_bytes=_WG_TILES + 256 * 128 * 4 - 1)), ("partial_floats", dict(partial_floats=384 * 128 - 1))], _BWD_BONE_ARGS),
    ("kasf_op_gcn_fwd", dict(dtype=0, batch=1, n_frames=4, mode=1, neighbour_num=4),
     _GCN + [("neighbour_num", dict(neighbour_num=0)), ("neighbour_num_big", dict(neighbour_num=5))], ()),
    ("kasf_op_gcn_bwd", dict(dtype=0, batch=1, n_frames=4, mode=1), _GCN, ()),
    ("kasf_op_gcn_bwd_rows", dict(dtype=0, batch=1, n_frames=4, mode=1, scratch_floats=128), _GCN + _SCRATCH, ("scratch",)),
    ("kasf_op_embed_bwd", dict(dtype=0, frames=1, scratch_floats=16), _DT + [("frames", dict(frames=0)), ("frames_big", dict(frames=2 ** 19))] + _SCRATCH,
     ("din3", "scratch")),
    ("kasf_op_gate_fwd", dict(dtype=0, M=1), _DT + [("tokens", dict(M=0)), ("tokens_big", dict(M=2 ** 23))], ("alpha",)),
    ("kasf_op_gate_bwd", dict(dtype=0, M=1, adaptive=1, scratch_floats=16), _DT + [("alpha_align", dict(alpha=OFF(4))), ("tokens", dict(M=0))] + _SCRATCH,
     ("g1", "g2", "scratch")),
    ("kasf_op_head_fwd", dict(dtype=0, M=1), _DT + [("tokens", dict(M=0))], ()),
    ("kasf_op_head_bwd", dict(dtype=0, M=1, scratch_floats=16), _DT + [("tokens", dict(M=0))] + _SCRATCH, ("scratch",)),
    ("kasf_op_rep_bwd", dict(dtype=0, M=1), _DT + [("tokens", dict(M=0))], ()),
    ("kasf_op_finalize_ls", dict(N=128, K=128), [("N", dict(N=64)), ("K", dict(K=256))], ()),
    ("kasf_op_add", dict(dtype=0, n=8), _DT + [("n", dict(n=7)), ("n_small", dict(n=0)), ("n_big", dict(n=2 ** 40))], ("c",)),
    ("kasf_op_cast", dict(dtype=0, n=8), _DT, ALL),
]

# (entry, message) of the refusals that no call from outside the library reaches on a machine without a device, each with its reason
UNREACHABLE = [
    ("kasf_op_dgrad_wg", "dgrad_wg: the launcher declined a form that kasf_dgrad_wg_supported accepts",
     "behind the launcher: the entry has asked kasf_dgrad_wg_supported about the same arguments before, and refuses what it does not accept"),
    ("kasf_op_wgrad_jobs", "wgrad_jobs: the launcher declined a call that passed every check",
     "behind the launcher: the entry restates the launcher's own conditions and split arithmetic, and refuses what it would decline"),
    ("kasf_op_attn_block_bwd", "attn_block_bwd: the launcher declined a call that passed every check",
     "behind the launcher: the entry has refused groups of more than 32 positions and every missing pointer before; a short sink is error 6, not this"),
    ("kasf_op_attn_block_bwd", "attn_block_bwd: the weight-gradient launcher declined a call that passed every check",
     "behind the second launcher: the entry restates its split arithmetic for partial_floats and passes it no fin job"),
    ("kasf_detect_boxes", "detect_boxes: the device refused the LDS size of the sort + NMS kernel",
     "comes back from the launcher, after its first kernel is on the stream: every host check has passed by then"),
]


def prototypes():
    """name -> (restype, [(parameter, ctypes type, is pointer)]) of every function that include/kasf.h declares."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "kasf.h")).read(), flags=re.S)
    scalar = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "double": C.c_double}
    out = {}
    for res, name, args in re.findall(r"^(int|int64_t)\s+(kasf_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.M | re.S):
        params = []
        for a in (s.strip() for s in args.split(",")):
            if a == "void":
                continue
            m = re.match(r"^(.*?)(\w+)(\[\d*\])?$", a)
            kind, pname, arr = m.group(1).strip(), m.group(2), m.group(3)
            pointer = "*" in kind or arr is not None
            params.append((pname, C.c_void_p if pointer else scalar[kind.replace("const", "").strip()], pointer))
        out[name] = (scalar[res], params)
    return out


def cases_of(entry):
    """[(case id, overrides, id of the case whose message it must repeat or None)] of one ENTRIES row: the written cases, then null:*, all_wrong and pair:*."""
    name, base, cases, nullable = entry
    params = PROTOS[name][1]
    cases = [c if len(c) == 3 else (*c, None) for c in cases]
    out = list(cases)
    if nullable != ALL:
        out += [(f"null:{p}", {p: None}, None) for p, _, ptr in params if ptr and p != "stream" and p not in nullable]
    out.append(("all_wrong", {p: (None if ptr else -1) for p, _, ptr in params}, None))
    for (a, ova, _), (b, ovb, _) in zip(cases, cases[1:]):
        if not set(ova) & set(ovb):
            out.append((f"pair:{a}+{b}", {**ova, **ovb}, a))
    return out


PROTOS = prototypes()


def _call(lib, name, base, overrides):
    res, params = PROTOS[name]
    unknown = (set(base) | set(overrides)) - {p for p, _, _ in params}
    assert not unknown, f"{name} has no parameter {sorted(unknown)}"
    keep, values = [], {}

    def fresh(offset=0):
        keep.append(C.create_string_buffer(BUF_BYTES + 64))
        return (C.addressof(keep[-1]) + 63) // 64 * 64 + offset

    def pointer(v):
        if v is None:
            return None
        if isinstance(v, _Marker):
            return fresh(v.arg if v.kind == "off" else 0)
        return C.addressof(v)

    spec = {**base, **overrides}
    for p, _, ptr in params:
        if ptr:
            v = spec.get(p, None if p == "stream" else BUF)
            values[p] = v if isinstance(v, _Marker) and v.kind == "same" else pointer(v)
        else:
            values[p] = spec.get(p, 0)
    for p, v in values.items():
        if isinstance(v, _Marker):
            values[p] = values[v.arg]
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = res, [t for _, t, _ in params]
    return int(fn(*[values[p] for p, _, _ in params]))


def replay(lib_path=LIB_PATH):
    """Runs every case against the library: [{"entry", "case", "code", "message"}] in table order.  Every call must be refused before it reaches a launch (a code
    that is non-zero and no HIP error, 1000 + hipError_t), and a pair case must repeat the message of its first half."""
    lib = C.CDLL(lib_path)
    lib.kasf_last_error.restype = C.c_char_p
    records = []
    for entry in ENTRIES:
        said = {}
        for cid, overrides, first in cases_of(entry):
            code = _call(lib, entry[0], entry[1], overrides)
            said[cid] = lib.kasf_last_error().decode()
            assert code != 0 and abs(code) < 1000, f"{entry[0]} {cid}: code {code} ({said[cid]}): the call was not refused"
            assert first is None or said[cid] == said[first], f"{entry[0]} {cid}: says {said[cid]!r}, not {said[first]!r}"
            records.append({"entry": entry[0], "case": cid, "code": code, "message": said[cid]})
    return records
