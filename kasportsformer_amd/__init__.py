"""kasportsformer_amd -- MI355X-native (gfx950) forward/backward path of KASportsFormer.

Public surface mirrors the reference's interface for this path:
  KASportsFormer, load_model            model/KASportsFormer.py:290, model/model_tools.py:79
  loss3, mpjpe_loss / ...               utils/loss_calc.py:6-27 (+ the train-step combination)
  loss7, LOSS7_NAMES                    utils/loss_calc.py:30-94, train_and_evaluate_sp.py:14-15,216-220 (the complete seven-term loss the yaml's six lambdas
                                        describe -- limb-length variance, limb length, limb angles, angle velocity on top of the three -- and its
                                        gradient in one launch; `train_one_epoch(lambda_limb_len=...)`)
  FusedAdamW                            optim.AdamW as used in train_and_evaluate_sp.py:270-272
  AdamW                                 the same as a `torch.optim.AdamW` subclass that takes parameters (the reference's `filter(requires_grad)` form): groups,
                                        subsets, `grad is None`, per-parameter steps, `lr_scheduler.*`, `max_grad_norm` clipping; one launch over a chunk table
  DataParallel                          nn.DataParallel replacement: one process per GPU, RCCL all-reduce
  joint_flip, predict_flip_tta,         utils/utilities.py:128-135, train_and_evaluate_sp.py:27-149, utils/error_calc.py:5-48
  clip_metrics, Evaluator, evaluate_one_epoch
  pack_clip_directory, PackedClips,     data/preprocessor/clip_generate_sp.py:28-79 (file format), data/reader/sp_dataset.py:45-92
  DeviceClipLoader
  train_one_epoch                       train_and_evaluate_sp.py:201-243
  warmup_lr, ReduceLROnPlateau          train_and_evaluate_sp.py:273,325-329,393-397
  checkpoint_save, checkpoint_load      utils/utilities.py:110-118, train_and_evaluate_sp.py:171-176,285-301
  slice_source, split_clips,            data/reader/sp_reader.py:25-169,205-249, data/reader/wp_reader.py:25-135,159-199 (offline clip slicing)
  mysplit_clips, resample
  lift_track, window_plan               demo/demo.py:132-156,194-254, demo/lib/utils.py:5-20 (2-D track -> 3-D poses; also
                                        `python -m kasportsformer_amd.lift`)
  lift_tracks                           the same over many tracks of different lengths in one batched call
  StreamLifter                          the same one frame at a time: per-player history on the device, one pose per player per tick
                                        (`python -m kasportsformer_amd.lift --online`)
  coco_to_h36m                          demo/lib/preprocess.py:10-69, demo/demo.py:75-78 (COCO-17 detector keypoints -> the H36M-17 layout, on the
                                        device; `layout="coco"` on the three lifts, `--layout coco`)
  heatmaps_to_keypoints                 demo/lib/hrnet/lib/utils/inference.py:21-82, demo/lib/hrnet/gen_kpts.py:158-161 (a top-down pose network's
                                        heatmaps -> COCO-17 or H36M-17 keypoints in image pixels, on the device; `StreamLifter.push_heatmaps`)
  heatmaps_to_keypoints(flipped=...)    demo/lib/hrnet/lib/utils/transforms.py:15-30, demo/lib/hrnet/experiments/w48_384x288_adam_lr1e-3.yaml:119-121 (the flip test:
                                        the network's output for the mirrored crops mirrored back, left / right maps swapped, shifted one column,
                                        averaged with the direct output in float32 and decoded, in one launch; `push_heatmaps(flipped=...)`)
  heatmaps_to_keypoints(decode=...),    not in the demo: DARK (Zhang et al., CVPR 2020) and DARK-UDP (Huang et al., CVPR 2020) sub-pixel refinement and the UDP
  gaussian_weights                      affine, what ViTPose and the *_dark / *_udp HRNet checkpoints are evaluated with, in the same one launch (a Gaussian blur
                                        and a logarithm around the argmax only, one Newton step; `push_heatmaps(decode=...)`)
  letterbox_frames, LetterboxResult     demo/lib/yolov3/preprocess.py:9-38, demo/lib/yolov3/human_detector.py:131 (video frames -> the YOLOv3 network's input, on the
                                        device: letterbox with bicubic resampling onto a canvas of 128, channel reversal, planes, / 255; one launch,
                                        reads the decoder's frame in place; its width / height are what `yolo_heads_to_boxes` takes)
  yuv_to_bgr, nv12_to_bgr, i420_to_bgr  demo/lib/hrnet/gen_kpts.py:106,118 (`cap.read()`'s colour conversion: a decoder's NV12 / I420 surface -> the uint8 BGR frame, on the
                                        device: nearest chroma, 20-bit fixed point, BT.601 / BT.709, limited / full range; one launch, reads the surface in
                                        place through its pitch; what `letterbox_frames` and `crop_persons` take)
  detections_to_boxes,                  demo/lib/yolov3/human_detector.py:116-168, demo/lib/yolov3/util.py:34-81,107-225, demo/lib/yolov3/bbox.py:51-78 (a YOLOv3
  yolo_heads_to_boxes, YOLOV3_ANCHORS   person detector's output -> person boxes in frame pixels, on the device: threshold, persons only, sort, greedy NMS,
                                        un-letterbox; what `heatmaps_to_keypoints(boxes=...)` takes)
  crop_persons                          demo/lib/hrnet/lib/utils/utilitys.py:139-169, demo/lib/hrnet/gen_kpts.py:152-157 (person boxes -> the pose network's
                                        normalised input crops, on the device: affine crop with bilinear sampling, ToTensor, Normalize, channel swap;
                                        its center / scale are what `heatmaps_to_keypoints` takes)
  SortTracker, TrackResult              demo/lib/sort/sort.py:15-222, demo/lib/hrnet/gen_kpts.py:111-148 (the demo's SORT tracker between the person boxes and the
                                        crops, on the device: fp64 Kalman filters, IoU, optimal assignment, births, deaths, ids; one launch per tick
                                        for every stream, takes `DetectResult` as it is, gives what `crop_persons` takes)
  TrackedLifter, TrackedTick            the seam between the two stages (demo/lib/hrnet/gen_kpts.py:125-170 hands each tracked person's keypoints to the lift):
                                        `SortTracker`'s ids and slots drive `StreamLifter`-style per-player histories on the device, births and deaths
                                        included; no read-back of the tracker's output, two launches and one forward per tick
  OneEuroFilter, smooth_tracks          not in the demo (its unused `revise_kpts`, demo/lib/preprocess.py:72-103, patches low-score leg joints): the One-Euro filter
                                        (Casiez et al., CHI 2012) over 2-D keypoints in front of the lift and 3-D poses behind it, state on the device, driven
                                        by host slot ids or by `TrackResult`, score-gated so that an occluded joint holds; one launch per tick, no read-back
                                        (`python -m kasportsformer_amd.lift --smooth`)
  refine_tracks                         not in the demo: what offline pose tooling does to a recorded track in front of the lift -- a joint that is not usable is
                                        interpolated between its usable neighbours (short leading and trailing runs hold), then a symmetric, zero-phase Gaussian
                                        over the known joints; parallel over frames, one launch (`python -m kasportsformer_amd.lift --refine`)
  fix_bone_lengths, bone_lengths,       not in the demo: one length per bone per player (the lower median over the track, or a measured table), re-imposed on every
  BoneLengthFilter                      frame by a walk from the root that keeps directions and the root; the bone table is utils/loss_calc.py:30-40's, the quantity
                                        what `loss_limb_var_calc` penalises; recorded tracks in three launches, live rows with a running mean per slot in one,
                                        driven by host slot ids or by `TrackResult` (`python -m kasportsformer_amd.lift --fix-bones`)
  place_poses, PlaceResult              not in the demo (it plots one person at the origin): the root translation that makes a root-relative pose re-project onto
                                        its keypoints through the camera's intrinsics, a 3 x 3 least-squares fit per frame in fp64 with Cauchy re-weighting and an
                                        optional metric scale from a bone table, so that several players stand where they stood; one launch, live and recorded
                                        (`python -m kasportsformer_amd.lift --place --camera FX,FY,CX,CY`)
  triangulate_keypoints,                not in the reference (it is monocular): one player's keypoint tracks in 2 to 16 calibrated cameras -> joints in the world
  undistort_keypoints, camera_row,      frame, per joint a 3 x 3 least-squares fit of the undistorted rays in fp64, re-weighted to pixels with the placement's Cauchy
  TriangulateResult                     weight, with the re-projection error per point and per view (a check on a lifted pose, labels for new footage); and the
                                        Brown-Conrady undistortion on its own, in front of `place_poses`; one launch each, one lane per joint
                                        (`python -m kasportsformer_amd.lift --place --camera-distortion K1,K2,P1,P2,K3`)
  match_players, match_costs,           not in the reference: which of the rows that several cameras' trackers emit are the same player -- the cost of a pair of
  match_groups, gather_matched,         rows is the mean gap between their keypoints' undistorted rays in pixels, in fp64 with every sum in a fixed order; the
  MatchResult                           cameras are then taken in turn, each one's rows assigned to the groups so far by the tracker's optimal assignment --
                                        and the tracks in group order, which is what `triangulate_keypoints` takes; three launches, nothing read back
  poses_to_world, DEMO_CAMERA_ROTATION  demo/lib/utils.py:55-73, demo/demo.py:242-248 (camera space -> world space, floor, unit scale; `--world`)
  draw_poses, bgr_to_nv12,              demo/demo.py:91-105,159-191,307-323, demo/lib/hrnet/lib/utils/utilitys.py:24-58 (`plot_on_frame`'s lines and dots over the frame, the
  poses_to_panel, DrawResult            score threshold, the 3-D plot's projection, and the frame as the NV12 surface an encoder takes, on the device: exact
                                        integer geometry -- not cv2's rasteriser --, 20-bit fixed-point BGR -> YUV; one launch, also in place)
"""
from .model import (KASportsFormer, load_model, set_single_stream, is_single_stream, set_deterministic, is_deterministic, set_fused_attention_backward,
                    is_fused_attention_backward)
from .functional import loss3, loss7, LOSS7_NAMES
from .optim import FusedAdamW, AdamW, plan_chunks
from .parallel import DataParallel
from .data import PackedClips, DeviceClipLoader, pack_clip_directory, read_clip_file, shard_indices
from .checkpoint import checkpoint_save, checkpoint_load, strip_module_prefix, adamw_state_dict, load_adamw_state_dict
from .loop import train_one_epoch
from .schedule import warmup_lr, apply_warmup, ReduceLROnPlateau
from .evaluate import joint_flip, predict_flip_tta, clip_metrics, Evaluator, evaluate_one_epoch
from .synthetic import synthetic_clips, synthetic_test_extras, teacher_labels, teacher_clips
from .slicing import slice_source, split_clips, mysplit_clips, resample
from .lift import lift_track, lift_tracks, window_plan
from .stream import StreamLifter
from .pose import coco_to_h36m, poses_to_world, DEMO_CAMERA_ROTATION
from .heatmap import heatmaps_to_keypoints, gaussian_weights
from .detect import detections_to_boxes, yolo_heads_to_boxes, DetectResult, YOLOV3_ANCHORS, YOLOV3_MASKS
from .crop import crop_persons, CropResult
from .letterbox import letterbox_frames, LetterboxResult
from .yuv import yuv_to_bgr, nv12_to_bgr, i420_to_bgr
from .draw import draw_poses, bgr_to_nv12, poses_to_panel, DrawResult
from .track import SortTracker, TrackResult, TrackState
from .tracked import TrackedLifter, TrackedTick
from .smooth import OneEuroFilter, smooth_tracks
from .refine import refine_tracks
from .bones import fix_bone_lengths, bone_lengths, BoneLengthFilter
from .place import place_poses, PlaceResult
from .triangulate import triangulate_keypoints, undistort_keypoints, camera_row, TriangulateResult
from .match import match_players, match_costs, match_groups, gather_matched, MatchResult, MatchCosts, MatchGroups

__all__ = ["KASportsFormer", "load_model", "set_single_stream", "is_single_stream", "set_deterministic", "is_deterministic", "set_fused_attention_backward", "is_fused_attention_backward", "loss3", "loss7", "LOSS7_NAMES", "FusedAdamW", "AdamW", "plan_chunks", "DataParallel", "joint_flip", "predict_flip_tta", "clip_metrics", "Evaluator",
           "evaluate_one_epoch", "PackedClips", "DeviceClipLoader", "pack_clip_directory", "read_clip_file", "shard_indices",
           "checkpoint_save", "checkpoint_load", "strip_module_prefix", "adamw_state_dict", "load_adamw_state_dict", "warmup_lr", "apply_warmup", "ReduceLROnPlateau", "train_one_epoch",
           "synthetic_clips", "synthetic_test_extras", "teacher_labels", "teacher_clips", "slice_source", "split_clips", "mysplit_clips", "resample",
           "lift_track", "lift_tracks", "window_plan", "StreamLifter", "coco_to_h36m", "poses_to_world", "DEMO_CAMERA_ROTATION", "heatmaps_to_keypoints", "gaussian_weights",
           "detections_to_boxes", "yolo_heads_to_boxes", "DetectResult", "YOLOV3_ANCHORS", "YOLOV3_MASKS", "crop_persons", "CropResult", "letterbox_frames", "LetterboxResult", "yuv_to_bgr", "nv12_to_bgr", "i420_to_bgr", "SortTracker", "TrackResult", "TrackState",
           "TrackedLifter", "TrackedTick", "OneEuroFilter", "smooth_tracks", "refine_tracks", "fix_bone_lengths", "bone_lengths", "BoneLengthFilter", "place_poses", "PlaceResult", "triangulate_keypoints", "undistort_keypoints", "camera_row", "TriangulateResult", "match_players", "match_costs", "match_groups", "gather_matched", "MatchResult", "MatchCosts", "MatchGroups", "draw_poses", "bgr_to_nv12", "poses_to_panel", "DrawResult"]
