"""Host side of the detector decode (kasportsformer_amd.detections_to_boxes / yolo_heads_to_boxes, kasf_detect_boxes): the numpy restatement the GPU tests hold
the kernels to (tests/test_gpu_detect.py imports it from here), tied to the fixture the reference's own predict_transform, write_results and un-letterbox wrote
(tests/golden/make_detect_golden.py); the prefix property of the caps; the refusals of the entry point and of the Python surface."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = np.float32, np.float64
GROUPS = ("a", "b")                                             # fixture groups: a = inp_dim 96 in 854 x 480, b = inp_dim 160 in 1080 x 1920
ANCHORS = ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
MASKS = ((6, 7, 8), (3, 4, 5), (0, 1, 2))


def fixture():
    return np.load(os.path.join(GOLDEN, "detect_decode.npz"), allow_pickle=False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _sigmoid(v):
    one = v.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-v))


def _first_max(v):
    """Rule 4's arg-max of the rows of v [n,C]: compared with > from class 0 on, so the first maximum wins, and a NaN neither wins nor, in first place, loses."""
    if v.shape[0] == 0:
        return np.zeros(0, np.int64)
    arg = np.argmax(np.where(np.isnan(v), -np.inf, v), axis=1)
    return np.where(np.isnan(v[:, 0]), 0, arg)


def heads_to_prediction_np(heads, inp_dim, anchors=ANCHORS, masks=MASKS, ft=F32):
    """Rules 1, 2 and 4 (heads form) -> (pred [B,N,6] = x, y, w, h, objectness, winning class score, arg [B,N] = winning class), in ``ft`` arithmetic:
    predict_transform (demo/lib/yolov3/util.py:34-81) per head, concatenated in the given order, with the class arg-max taken on the logits."""
    preds, args = [], []
    for head, mask in zip(heads, masks):
        t = np.asarray(head)
        t = t if t.dtype == ft else t.astype(ft)                # fp16 widens exactly; bf16 reaches here as float32 already
        B, ch, G, _ = t.shape
        A = len(mask)
        stride = inp_dim // G
        assert inp_dim % G == 0 and ch % A == 0
        anc = np.array([[anchors[i][0] / stride, anchors[i][1] / stride] for i in mask], dtype=F64).astype(F32).astype(ft)   # FloatTensor(a / stride)
        t = t.reshape(B, A, ch // A, G * G).transpose(0, 3, 1, 2)                                                              # [B, cell, a, attr]
        cell = np.arange(G * G)
        cx, cy = (cell % G).astype(ft)[None, :, None], (cell // G).astype(ft)[None, :, None]
        st = ft(stride)
        with np.errstate(over="ignore"):
            x = (_sigmoid(t[..., 0]) + cx) * st
            y = (_sigmoid(t[..., 1]) + cy) * st
            w = np.exp(t[..., 2]) * anc[None, None, :, 0] * st
            h = np.exp(t[..., 3]) * anc[None, None, :, 1] * st
        obj = _sigmoid(t[..., 4])
        logits = t[..., 5:].reshape(B * G * G * A, -1)
        arg = _first_max(logits)
        cls = _sigmoid(logits[np.arange(len(arg)), arg]).reshape(B, G * G, A)
        preds.append(np.stack((x, y, w, h, obj, cls), axis=-1).reshape(B, G * G * A, 6))
        args.append(arg.reshape(B, G * G * A))
    return np.concatenate(preds, axis=1), np.concatenate(args, axis=1)


def prediction_rows_np(prediction, ft=F32):
    """Rule 4 (prediction form) -> the same pair from prediction [B,N,5+C]."""
    p = np.asarray(prediction)
    p = p if p.dtype == ft else p.astype(ft)
    B, N, _ = p.shape
    scores = p[..., 5:].reshape(B * N, -1)
    arg = _first_max(scores)
    cls = scores[np.arange(B * N), arg].reshape(B, N, 1)
    return np.concatenate((p[..., :5], cls), axis=2), arg.reshape(B, N)


def _iou(p, q, ft):
    """bbox_iou (demo/lib/yolov3/bbox.py:51-78) of box p [4] against boxes q [n,4], one ``ft`` operation at a time."""
    one, zero = ft(1), ft(0)
    ix1, iy1 = np.maximum(p[0], q[:, 0]), np.maximum(p[1], q[:, 1])
    ix2, iy2 = np.minimum(p[2], q[:, 2]), np.minimum(p[3], q[:, 3])
    inter = np.maximum(ix2 - ix1 + one, zero) * np.maximum(iy2 - iy1 + one, zero)
    a1 = (p[2] - p[0] + one) * (p[3] - p[1] + one)
    a2 = (q[:, 2] - q[:, 0] + one) * (q[:, 3] - q[:, 1] + one)
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (a1 + a2 - inter)


def detect_decode_np(src, width, height, inp_dim, *, form="prediction", anchors=ANCHORS, masks=MASKS, confidence=0.70, nms=0.4, class_id=0, max_boxes=32,
                     max_candidates=1024, ft=F32, trace=None):
    """Rules 1-9 of include/kasf.h's kasf_detect_boxes in numpy, one ``ft`` (float32; float64 for the fixture's second opinion) operation at a time, in
    the reference's order -> (boxes [B,max_boxes,6] ft, count [B] int32, candidates [B] int32, index [B,max_boxes] int32).  ``trace``: a list that receives
    (image, IoU) of every pair NMS compares (tests/golden/make_detect_golden.py checks the fixture's margins with it)."""
    pred, arg = heads_to_prediction_np(src, inp_dim, anchors, masks, ft) if form == "heads" else prediction_rows_np(src, ft)
    B, N, _ = pred.shape
    wv, hv = np.broadcast_to(np.asarray(width, F64), (B,)).astype(F32).astype(ft), np.broadcast_to(np.asarray(height, F64), (B,)).astype(F32).astype(ft)
    conf, thr, inp, two, zero = ft(F32(confidence)), ft(F32(nms)), ft(inp_dim), ft(2), ft(0)
    boxes, index = np.zeros((B, max_boxes, 6), ft), np.full((B, max_boxes), -1, np.int32)
    count, cands = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        p = pred[b]
        with np.errstate(invalid="ignore", over="ignore"):
            passing = p[:, 4] > conf                                                           # rule 3 (a NaN fails)
            corners = np.stack((p[:, 0] - p[:, 2] / two, p[:, 1] - p[:, 3] / two, p[:, 0] + p[:, 2] / two, p[:, 1] + p[:, 3] / two), axis=1)   # rule 5
        keep = passing & (arg[b] == class_id) & np.isfinite(corners).all(axis=1)               # rules 4 and 10
        idx = np.nonzero(keep)[0]
        cands[b] = len(idx)
        idx = idx[np.lexsort((idx, -p[idx, 4]))][:max_candidates]                              # rules 6 and 9
        c = corners[idx]
        dead = np.zeros(len(idx), bool)
        kept = []
        for i in range(len(idx)):                                                              # rule 7
            if dead[i]:
                continue
            kept.append(i)
            if len(kept) == max_boxes:
                break
            iou = _iou(c[i], c[i + 1:], ft)
            if trace is not None:
                trace.extend((b, float(v)) for v in iou[~dead[i + 1:]])
            with np.errstate(invalid="ignore"):
                dead[i + 1:] |= ~(iou < thr)
        n = len(kept)
        one = ft(1)                                                                            # rule 8; torch evaluates `number / tensor` as reciprocal * number
        sf = np.minimum(one / wv[b] * inp, one / hv[b] * inp)
        padx, pady = (inp - sf * wv[b]) / two, (inp - sf * hv[b]) / two
        k = c[kept]
        boxes[b, :n, 0] = np.minimum(np.maximum((k[:, 0] - padx) / sf, zero), wv[b])
        boxes[b, :n, 1] = np.minimum(np.maximum((k[:, 1] - pady) / sf, zero), hv[b])
        boxes[b, :n, 2] = np.minimum(np.maximum((k[:, 2] - padx) / sf, zero), wv[b])
        boxes[b, :n, 3] = np.minimum(np.maximum((k[:, 3] - pady) / sf, zero), hv[b])
        boxes[b, :n, 4:] = p[idx[kept], 4:6]
        index[b, :n] = idx[kept]
        count[b] = n
    return boxes, count, cands, index


def group(fx, g):
    heads = [fx[f"{g}_head{k}"] for k in range(3)]
    return heads, fx[f"{g}_prediction"], float(fx[f"{g}_frame"][0]), float(fx[f"{g}_frame"][1]), int(fx[f"{g}_inp_dim"])


KW = dict(confidence=0.30, nms=0.4)


@pytest.mark.parametrize("g", GROUPS)
def test_restatement_equals_the_reference_on_its_prediction(g):
    fx = fixture()
    heads, pred, w, h, inp = group(fx, g)
    assert pred.dtype == F32 and pred.shape[0] == 3 and pred.shape[2] == 85
    boxes, count, cands, index = detect_decode_np(pred, w, h, inp, **KW)
    assert boxes.dtype == F32
    assert np.array_equal(count, fx[f"{g}_ref_count"]) and (count >= 5).all() and (cands - count >= 2).all()
    assert np.array_equal(index, fx[f"{g}_ref_index"]), "survivors and their order"
    assert same_bits(boxes, fx[f"{g}_ref_boxes"]), "every operation is a single fp32 operation: the reference's rows bit for bit"
    assert np.array_equal(cands, fx[f"{g}_candidates"])
    for b in range(3):
        assert (index[b, count[b]:] == -1).all() and not boxes[b, count[b]:].any()
    clipped = (boxes[..., 0] == 0) | (boxes[..., 1] == 0) | (boxes[..., 2] == F32(w)) | (boxes[..., 3] == F32(h))
    assert (clipped.sum(axis=1) >= 1).all(), "every image has a box that reaches outside the frame"


@pytest.mark.parametrize("g", GROUPS)
def test_restatement_on_the_heads_is_the_reference_within_its_own_error(g):
    fx = fixture()
    heads, pred, w, h, inp = group(fx, g)
    assert all(hd.dtype == np.float16 for hd in heads) and [hd.shape[2] for hd in heads] == [inp // 32, inp // 16, inp // 8]
    boxes, count, cands, index = detect_decode_np(heads, w, h, inp, form="heads", **KW)
    assert np.array_equal(count, fx[f"{g}_ref_count"]) and np.array_equal(index, fx[f"{g}_ref_index"]) and np.array_equal(cands, fx[f"{g}_candidates"])
    exy, esc = float(fx[f"{g}_ref_err_xy"]), float(fx[f"{g}_ref_err_score"])
    assert 0 < exy < 1e-3 and 0 <= esc < 1e-6, "the reference's own fp32 chain sits about an ulp of the coordinate from the fp64 evaluation"
    f64 = fx[f"{g}_f64_boxes"]
    assert np.array_equal(fx[f"{g}_f64_index"], index) and np.array_equal(fx[f"{g}_f64_count"], count)
    dxy, dsc = np.abs(boxes[..., :4] - f64[..., :4]).max(), np.abs(boxes[..., 4:] - f64[..., 4:]).max()
    print(f"group {g}: restatement - fp64 xy {dxy:.3e} (reference {exy:.3e}), scores {dsc:.3e} (reference {esc:.3e})")
    assert dxy <= 4 * exy and dsc <= 4 * esc
    # ... and the fixture's prediction is predict_transform of the fixture's heads: x, y, w, h, objectness within a few ulp of this restatement's chain
    mine, arg = heads_to_prediction_np(heads, inp)
    assert np.allclose(mine[..., :5], pred[..., :5], rtol=1e-5, atol=1e-6)
    assert np.array_equal(arg, np.argmax(pred[..., 5:], axis=2))


@pytest.mark.parametrize("g", GROUPS)
def test_capped_results_are_prefixes(g):
    fx = fixture()
    heads, pred, w, h, inp = group(fx, g)
    full = detect_decode_np(pred, w, h, inp, **KW)
    n, c = full[1], full[2]
    for mc in (1, 3, int(c.min()) - 1, int(c.max())):
        boxes, count, cands, index = detect_decode_np(pred, w, h, inp, max_candidates=mc, **KW)
        assert np.array_equal(cands, c), "candidates reports the uncapped number"
        for b in range(3):
            m = count[b]
            assert 1 <= m <= n[b] and np.array_equal(index[b, :m], full[3][b, :m]) and same_bits(boxes[b, :m], full[0][b, :m])
            assert m == n[b] or mc < c[b]
    for mb in (1, 2, int(n.min()) - 1):
        boxes, count, cands, index = detect_decode_np(pred, w, h, inp, max_boxes=mb, **KW)
        assert boxes.shape == (3, mb, 6) and (count == mb).all() and np.array_equal(cands, c)
        assert np.array_equal(index, full[3][:, :mb]) and same_bits(boxes, full[0][:, :mb])


def test_ties_chains_and_dropped_rows():
    """The hand-made rows tests/test_gpu_detect.py runs on the device: what the rules say about them."""
    pred, expect = tie_rows()
    boxes, count, cands, index = detect_decode_np(pred, 64, 64, 64, confidence=0.25, nms=0.5, max_boxes=16)
    assert count[0] == len(expect) and index[0, :count[0]].tolist() == expect and cands[0] == 8


def tie_rows():
    """prediction [1,12,8] (C = 3) with integer-valued boxes, and the candidate indices rule 6 + 7 keep, in order (nms = 0.5, confidence = 0.25).
    IoU with the + 1 of bbox_iou: boxes of side s cover s + 1; two 9 x 9 boxes (side 8) shifted by 3 in x overlap 6 x 9 = 54 of 81 + 81 - 54 = 108: exactly 0.5."""
    def row(cx, cy, w, h, obj, cls=(0.9, 0.1, 0.1)):
        return [cx, cy, w, h, obj, *cls]
    rows = [
        row(10, 10, 8, 8, 0.75),                    # 0  ties with 1 on objectness: lower index first; kept
        row(40, 10, 8, 8, 0.75),                    # 1  kept, second
        row(13, 10, 8, 8, 0.5),                     # 2  IoU with 0 exactly 0.5 = nms: suppressed
        row(10, 40, 8, 8, 0.625),                   # 3  A: kept
        row(12, 40, 8, 8, 0.5625),                  # 4  B: IoU with A = 63 / 99 > 0.5: suppressed
        row(15, 40, 8, 8, 0.53125),                 # 5  C: IoU with A = 36 / 126 < 0.5 survives, though B (63 / 99... shifted 3: 0.5) would have suppressed it
        row(40, 40, 8, 8, 0.875, (0.5, 0.5, 0.25)),  # 6  class tie: the first maximum is class 0: kept, first of all
        row(40, 40, 8, 8, 0.9, (0.5, 0.75, 0.25)),   # 7  class 1 wins: not a person
        row(50, 50, 8, 8, float("nan")),            # 8  NaN objectness: dropped
        row(50, 50, float("inf"), 8, 0.95),         # 9  non-finite box: dropped
        row(20, 20, 8, 8, 0.25),                    # 10 objectness == confidence: the comparison is strict
        row(60, 60, 8, 8, 0.3125, (float("nan"), 0.9, 0.1)),   # 11 a NaN in first place is not beaten: class 0, kept, last
    ]
    return np.array([rows], F32), [6, 0, 1, 3, 5, 11]


def test_sixteen_bit_inputs_are_widened_exactly():
    fx = fixture()
    heads, pred, w, h, inp = group(fx, "a")
    a = detect_decode_np(heads, w, h, inp, form="heads", **KW)
    b = detect_decode_np([hd.astype(F32) for hd in heads], w, h, inp, form="heads", **KW)
    assert all(same_bits(x, y) for x, y in zip(a, b))


def test_symbols_and_workspace_query():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    for name in ("kasf_detect_boxes", "kasf_detect_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == lib.kasf_version() == 12
    q = lib.kasf_detect_workspace_bytes
    assert q(0, 10, 1) == 0 and q(1, 1, 1) > 0
    last = 0
    for B, N, K in ((1, 567, 1), (1, 567, 1024), (1, 1575, 1024), (3, 1575, 1024), (3, 10647, 2048), (64, 10647, 4096), (65535, 1 << 24, 4096)):
        now = q(B, N, K)
        assert now >= last and now >= B * N * 28, (B, N, K)
        last = now
    for bad in ((-1, 10, 1), (65536, 10, 1), (1, 0, 1), (1, (1 << 24) + 1, 1), (1, 10, 0), (1, 10, 4097)):
        assert q(*bad) == -2 and lib.kasf_last_error(), bad
    assert _lib.DETECT_MAX_CANDIDATES == 4096 >= 2048


def test_entry_point_refuses_without_a_device():
    from kasportsformer_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "kasf.h")).read()
    assert "int kasf_detect_boxes(const void* const* src, int32_t n_src, int32_t form, int32_t dtype, int32_t batch," in hdr
    C_, A, G, B, MB = 3, 2, 4, 2, 4
    N = G * G * A
    src = np.full(B * A * (5 + C_) * G * G, 3, F32)
    anchors, wh = np.full(A * 2, 5, F32), np.full(B * 2, 7, F32)
    boxes, index, count = np.full(B * MB * 6, 9, F32), np.full(B * MB, 11, np.int32), np.full(B * 2, 13, np.int32)
    nbytes = lib.kasf_detect_workspace_bytes(B, N, 8)
    ws = np.full(nbytes, 15, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    srcs, nosrc = (C.c_void_p * 4)(vp(src), vp(src), vp(src), vp(src)), (C.c_void_p * 4)(None, None, None, None)
    grid, bigrid = (C.c_int32 * 4)(G, G, G, G), (C.c_int32 * 4)(N, 0, 0, 0)
    anc = anchors.ctypes.data_as(C.POINTER(C.c_float))
    f = lib.kasf_detect_boxes

    def call(src=srcs, n_src=1, form=1, dtype=0, batch=B, grid=grid, A=A, C=C_, anchors=anc, inp_dim=32, wh=vp(wh), confidence=0.5, nms=0.4, class_id=0,
             mc=8, mb=MB, boxes=vp(boxes), index=vp(index), count=vp(count), ws=vp(ws), nbytes=nbytes):
        return f(src, n_src, form, dtype, batch, grid, A, C, anchors, inp_dim, wh, confidence, nms, class_id, mc, mb, boxes, index, count, ws, nbytes, None)

    assert call(batch=0) == 0 and call(batch=0, src=nosrc, wh=None, boxes=None, index=None, count=None, ws=None, nbytes=0) == 0     # nothing to do
    refused = [dict(src=None), dict(src=nosrc), dict(grid=None), dict(anchors=None), dict(wh=None), dict(boxes=None), dict(index=None), dict(count=None),
               dict(ws=None), dict(batch=-1), dict(batch=65536), dict(n_src=0), dict(n_src=5), dict(n_src=-1), dict(form=0, n_src=2, grid=bigrid),
               dict(A=0), dict(A=9), dict(C=0), dict(C=-3), dict(class_id=-1), dict(class_id=C_), dict(inp_dim=30), dict(inp_dim=0), dict(inp_dim=-32),
               dict(grid=(C.c_int32 * 4)(0, G, G, G)), dict(n_src=2, grid=(C.c_int32 * 4)(G, 5, G, G)), dict(mc=0), dict(mc=4097), dict(mb=0), dict(mb=9),
               dict(confidence=float("nan")), dict(confidence=float("inf")), dict(nms=float("nan")), dict(nms=float("-inf")), dict(nbytes=nbytes - 1),
               dict(nbytes=0), dict(form=2), dict(form=-1), dict(dtype=3), dict(dtype=-1), dict(form=0, grid=(C.c_int32 * 4)(0, 0, 0, 0)),
               dict(form=0, grid=bigrid, boxes=None), dict(form=0, grid=bigrid, C=0)]
    for kw in refused:
        assert call(**kw) == 2, kw
        assert lib.kasf_last_error(), kw
    assert (src == 3).all() and (anchors == 5).all() and (wh == 7).all() and (boxes == 9).all() and (index == 11).all() and (count == 13).all()
    assert (ws == 15).all(), "a refused call touches no buffer"


def test_python_surface_refuses_before_any_launch():
    import kasportsformer_amd as K
    for name in ("detections_to_boxes", "yolo_heads_to_boxes", "YOLOV3_ANCHORS"):
        assert name in K.__all__ and name in K.__doc__
    assert tuple(K.YOLOV3_ANCHORS) == ANCHORS and tuple(K.YOLOV3_MASKS) == MASKS
    assert "0.30" in K.detections_to_boxes.__doc__ and "0.30" in K.yolo_heads_to_boxes.__doc__
    pred = np.zeros((2, 10, 85), F32)
    heads = [np.zeros((2, 255, g, g), np.float16) for g in (2, 4, 8)]
    d, y = K.detections_to_boxes, K.yolo_heads_to_boxes
    with pytest.raises(RuntimeError):
        d(pred, 100, 100, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            d(pred, 100, 100)
        with pytest.raises(RuntimeError, match="no CPU path"):
            y(heads, np.array([100, 200]), torch.tensor([50.0, 60.0]), 64)
    for exc, call in ((TypeError, lambda: d(pred.astype(F64), 100, 100)),
                      (TypeError, lambda: d(pred.tolist(), 100, 100)),
                      (TypeError, lambda: d(torch.zeros((2, 10, 85), dtype=torch.int32), 100, 100)),
                      (TypeError, lambda: d(pred, "wide", 100)),
                      (TypeError, lambda: y(heads[0], 100, 100, 64)),
                      (TypeError, lambda: y([heads[0], heads[1].astype(F32)], 100, 100, 64, masks=MASKS[:2])),
                      (ValueError, lambda: d(pred[0], 100, 100)),
                      (ValueError, lambda: d(pred[:, :, :5], 100, 100)),
                      (ValueError, lambda: d(pred[:, :0], 100, 100)),
                      (ValueError, lambda: d(pred, 0, 100)),
                      (ValueError, lambda: d(pred, 100, -1)),
                      (ValueError, lambda: d(pred, 100, float("nan"))),
                      (ValueError, lambda: d(pred, [100, 100, 100], 100)),
                      (ValueError, lambda: d(pred, 100, 100, 0)),
                      (ValueError, lambda: d(pred, 100, 100, confidence=float("nan"))),
                      (ValueError, lambda: d(pred, 100, 100, nms=float("inf"))),
                      (ValueError, lambda: d(pred, 100, 100, class_id=80)),
                      (ValueError, lambda: d(pred, 100, 100, class_id=-1)),
                      (ValueError, lambda: d(pred, 100, 100, max_candidates=0)),
                      (ValueError, lambda: d(pred, 100, 100, max_candidates=4097)),
                      (ValueError, lambda: d(pred, 100, 100, max_boxes=0)),
                      (ValueError, lambda: d(pred, 100, 100, max_boxes=9, max_candidates=8)),
                      (ValueError, lambda: y([], 100, 100, 64)),
                      (ValueError, lambda: y(heads * 2, 100, 100, 64, masks=MASKS * 2)),
                      (ValueError, lambda: y(heads, 100, 100, 60)),
                      (ValueError, lambda: y(heads, 100, 100, 64, masks=MASKS[:2])),
                      (ValueError, lambda: y(heads, 100, 100, 64, masks=((6, 7), (3, 4, 5), (0, 1, 2)))),
                      (ValueError, lambda: y(heads, 100, 100, 64, masks=((6, 7, 9), (3, 4, 5), (0, 1, 2)))),
                      (ValueError, lambda: y(heads, 100, 100, 64, num_classes=20)),
                      (ValueError, lambda: y(heads, 100, 100, 64, num_classes=0)),
                      (ValueError, lambda: y(heads, 100, 100, 64, anchors=((10, 13), (0, 5)))),
                      (ValueError, lambda: y([heads[0], heads[1][:1]], 100, 100, 64, masks=MASKS[:2])),
                      (ValueError, lambda: y([heads[0][:, :, :, :1]], 100, 100, 64, masks=MASKS[:1]))):
        with pytest.raises(exc):
            call()
    assert not pred.any() and not any(h.any() for h in heads)
