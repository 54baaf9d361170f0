"""The detector decode on the device (kasf_detect_boxes, K.detections_to_boxes, K.yolo_heads_to_boxes) against the reference's own rows in
tests/golden/detect_decode.npz and against the numpy restatement of tests/test_detect_cpu.py, which that file ties to them.

Prediction form: device and restatement perform the same IEEE fp32 operations, so every comparison is on the bits.  Heads form: the device's exp is not the
host's, so survivors and order are compared exactly (the inputs keep the fixture's margins: no decision hangs on a last bit) and coordinates / scores against the
float64 evaluation of the same rules, within 4 x the distance at which the reference's own fp32 chain sits from it in the fixture (ref_err_xy, ref_err_score:
about one ulp of a coordinate of a 854- or 1,920-pixel frame).  The generated cases use 854 x 480 frames, so they take group a's figures.  A wrong anchor,
stride, + 1 or half-pixel is thousands of times that.  Nothing here provokes a fault."""
import numpy as np
import pytest
import torch

import kasportsformer_amd as K
from tests.test_detect_cpu import ANCHORS, F32, F64, GROUPS, KW, _sigmoid, detect_decode_np, fixture, group, heads_to_prediction_np, tie_rows

pytestmark = pytest.mark.gpu

_FIXTURE = {}


def golden():
    if not _FIXTURE:
        fx = fixture()
        _FIXTURE.update({k: fx[k] for k in fx.files})
    return _FIXTURE


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def same(result, want) -> bool:
    """A DetectResult against the restatement's (boxes, count, candidates, index): the same bits (a NaN class score included)."""
    boxes, count, cands, index = want
    return (tuple(result.boxes.shape) == boxes.shape and bits(result.boxes) == np.ascontiguousarray(boxes, F32).tobytes()
            and bits(result.count) == count.astype(np.int32).tobytes() and bits(result.candidates) == cands.astype(np.int32).tobytes()
            and bits(result.index) == np.ascontiguousarray(index, np.int32).tobytes())


def close(result, want64, exy, esc):
    """Same survivors in the same order; coordinates and scores within 4 x the reference's own distance from the float64 values."""
    boxes, count, cands, index = want64
    assert bits(result.count) == count.tobytes() and bits(result.index) == index.tobytes() and bits(result.candidates) == cands.tobytes()
    got = result.boxes.cpu().numpy().astype(F64)
    dxy, dsc = np.abs(got[..., :4] - boxes[..., :4]).max(), np.abs(got[..., 4:] - boxes[..., 4:]).max()
    print(f"device - fp64: xy {dxy:.3e} (bar {4 * exy:.3e}), scores {dsc:.3e} (bar {4 * esc:.3e})")
    assert dxy <= 4 * exy and dsc <= 4 * esc


def masks_for(n_heads, A):
    return (((6, 7, 8), (3, 4, 5), (0, 1, 2)) if A == 3 else ((8,), (4,), (0,)))[:n_heads]


def make_heads(seed, B, inp, n_heads, A, C, conf=0.30, nms=0.4):
    """Random fp16-representable heads with ~14 planted persons per image (some in neighbouring cells, so NMS has work), 3 planted other objects when C > 1,
    re-drawn until the fixture's margins hold: |objectness - confidence| >= 1e-3, objectness gaps >= 1e-4, |iou - nms| >= 1e-3, class logit margin >= 0.05."""
    grids, masks = [inp // 32, inp // 16, inp // 8][:n_heads], masks_for(n_heads, A)
    for attempt in range(50):
        g = np.random.default_rng(1000 * seed + attempt)
        heads = []
        for G in grids:
            t = g.normal(size=(B, A, 5 + C, G, G))
            t[:, :, 2:4] *= 0.4
            t[:, :, 4] = t[:, :, 4] * 0.5 - 6.0
            t[:, :, 5:] = t[:, :, 5:] - 4.0
            heads.append(t)
        for b in range(B):
            objs = list(g.permutation(np.arange(-0.3, 3.6, 0.06)))
            for n in range(14):
                k = int(g.integers(0, n_heads))
                G = grids[k]
                a, cy, cx = int(g.integers(0, A)), int(g.integers(0, G)), int(g.integers(0, G))
                for dx in ((0, 1) if n % 3 == 0 and cx + 1 < G else (0,)):       # a duplicate in the next cell
                    t = heads[k]
                    t[b, a, 4, cy, cx + dx] = objs.pop()
                    t[b, a, 0, cy, cx + dx] = 2.0 if dx == 0 else -2.0
                    t[b, a, 2:4, cy, cx + dx] = np.log(0.3 * inp / np.array(ANCHORS[masks[k][a]])) + g.normal(size=2) * 0.05
                    t[b, a, 5:, cy, cx + dx] = np.minimum(t[b, a, 5:, cy, cx + dx], -1.0)
                    t[b, a, 5 + (0 if n < 11 or C == 1 else 1 + n % (C - 1)), cy, cx + dx] = 4.0
        heads = [t.reshape(B, A * (5 + C), t.shape[3], t.shape[4]).astype(np.float16) for t in heads]
        pred64, arg = heads_to_prediction_np(heads, inp, masks=masks, ft=F64)
        trace = []
        want64 = detect_decode_np(heads, 854, 480, inp, form="heads", masks=masks, confidence=conf, nms=nms, ft=F64, trace=trace)
        obj = pred64[..., 4]
        ok = np.abs(obj - F64(F32(conf))).min() >= 1e-3 and (not trace or np.abs(np.array([v for _, v in trace]) - F64(F32(nms))).min() >= 1e-3)
        for b in range(B):
            person = (obj[b] > conf) & (arg[b] == 0)
            o = np.sort(obj[b][person])
            ok = ok and (len(o) < 2 or np.diff(o).min() >= 1e-4)
            if C > 1:
                rows = np.concatenate([h[b].astype(F64).reshape(A, 5 + C, -1).transpose(2, 0, 1).reshape(-1, 5 + C) for h in heads])[obj[b] > conf, 5:]
                top2 = np.sort(rows, axis=1)[:, -2:]
                ok = ok and (top2[:, 1] - top2[:, 0]).min() >= 0.05
        if ok and (want64[1] >= 3).all() and (want64[2] > want64[1]).any():
            return heads, masks, want64
    raise AssertionError("no draw met the margins")


def full_prediction(heads, inp, masks):
    """[B,N,5+C] float32 as predict_transform leaves it (numpy's exp): the first five columns of the restatement and the sigmoid of every class logit."""
    pred, _ = heads_to_prediction_np(heads, inp, masks=masks)
    cls = []
    for h, m in zip(heads, masks):
        B, ch, G, _ = h.shape
        A = len(m)
        t = h.astype(F32).reshape(B, A, ch // A, G * G).transpose(0, 3, 1, 2).reshape(B, G * G * A, ch // A)
        cls.append(_sigmoid(t[..., 5:]))
    return np.ascontiguousarray(np.concatenate((pred[..., :5], np.concatenate(cls, axis=1)), axis=2))


@pytest.mark.parametrize("g", GROUPS)
def test_fixture_prediction_form_is_the_reference_bit_for_bit(g):
    fx = golden()
    heads, pred, w, h, inp = group(fx, g)
    x = torch.from_numpy(pred).cuda()
    before = x.clone()
    r = K.detections_to_boxes(x, w, h, inp, **KW)
    assert r.boxes.is_cuda and r.boxes.dtype == torch.float32 and tuple(r.boxes.shape) == (3, 32, 6) and r.count.dtype == torch.int32
    assert same(r, (fx[f"{g}_ref_boxes"], fx[f"{g}_ref_count"], fx[f"{g}_candidates"], fx[f"{g}_ref_index"]))
    assert torch.equal(r.boxes, torch.from_numpy(fx[f"{g}_ref_boxes"]).cuda()) and torch.equal(r.index, torch.from_numpy(fx[f"{g}_ref_index"]).cuda())
    assert torch.equal(x, before), "the input is only read"
    assert same(K.detections_to_boxes(pred, w, h, inp, **KW), (fx[f"{g}_ref_boxes"], fx[f"{g}_ref_count"], fx[f"{g}_candidates"], fx[f"{g}_ref_index"])), "host input"


@pytest.mark.parametrize("g", GROUPS)
def test_fixture_heads_form(g):
    fx = golden()
    heads, pred, w, h, inp = group(fx, g)
    hs = [torch.from_numpy(hd).cuda() for hd in heads]
    before = [t.clone() for t in hs]
    r = K.yolo_heads_to_boxes(hs, w, h, inp, **KW)
    assert np.array_equal(fx[f"{g}_f64_count"], fx[f"{g}_ref_count"]) and np.array_equal(fx[f"{g}_f64_index"], fx[f"{g}_ref_index"])
    close(r, (fx[f"{g}_f64_boxes"], fx[f"{g}_ref_count"], fx[f"{g}_candidates"], fx[f"{g}_ref_index"]), float(fx[f"{g}_ref_err_xy"]), float(fx[f"{g}_ref_err_score"]))
    assert all(torch.equal(a, b) for a, b in zip(hs, before))
    n = r.count.cpu().numpy()
    for b in range(3):
        assert not r.boxes[b, n[b]:].any() and (r.index[b, n[b]:] == -1).all()


def test_sixteen_bit_inputs_give_the_fp32_result_of_the_widened_values():
    fx = golden()
    heads, pred, w, h, inp = group(fx, "a")
    for dt in (torch.float16, torch.bfloat16):
        hs = [torch.from_numpy(hd.astype(F32)).cuda().to(dt) for hd in heads]          # bf16: rounds the fp16 values once more; then exact
        narrow = K.yolo_heads_to_boxes(hs, w, h, inp, **KW)
        wide = K.yolo_heads_to_boxes([t.float() for t in hs], w, h, inp, **KW)
        assert all(bits(a) == bits(b) for a, b in zip(narrow, wide)), dt
        assert int(narrow.count.sum()) > 0
        p = torch.from_numpy(pred).cuda().to(dt)
        narrow, wide = K.detections_to_boxes(p, w, h, inp, **KW), K.detections_to_boxes(p.float(), w, h, inp, **KW)
        assert all(bits(a) == bits(b) for a, b in zip(narrow, wide)), dt
        assert same(wide, detect_decode_np(p.float().cpu().numpy(), w, h, inp, **KW))


#                        inp  heads B  C   A  view
@pytest.mark.parametrize("inp,n_heads,B,C,A,view", [(64, 3, 1, 80, 3, False), (96, 2, 3, 20, 3, False), (160, 1, 5, 1, 1, False), (64, 3, 5, 20, 1, False),
                                                    (416, 3, 1, 80, 3, False), (96, 3, 3, 80, 3, True), (160, 2, 1, 1, 3, False)])
def test_shape_tails_against_the_restatement(inp, n_heads, B, C, A, view):
    fx = golden()
    heads, masks, want64 = make_heads(inp + 7 * B + C, B, inp, n_heads, A, C)
    kw = dict(confidence=0.30, nms=0.4)
    if view:                                                                    # every second image / every second row of a larger tensor
        hs = []
        for hd in heads:
            big = torch.zeros((2 * B,) + hd.shape[1:], dtype=torch.float16, device="cuda")
            big[::2] = torch.from_numpy(hd).cuda()
            hs.append(big[::2])
            assert not hs[-1].is_contiguous()
    else:
        hs = [torch.from_numpy(hd).cuda() for hd in heads]
    r = K.yolo_heads_to_boxes(hs, 854, 480, inp, masks=masks, num_classes=C, **kw)
    close(r, want64, float(fx["a_ref_err_xy"]), float(fx["a_ref_err_score"]))
    pred = full_prediction(heads, inp, masks)
    want = detect_decode_np(pred, 854, 480, inp, **kw)
    assert np.array_equal(want[3], want64[3]), "the generated case keeps its margins in fp32 too"
    if view:
        big = torch.zeros((B, pred.shape[1], 2 * pred.shape[2]), device="cuda")
        big[:, :, ::2] = torch.from_numpy(pred).cuda()
        x = big[:, :, ::2]
        assert not x.is_contiguous()
    else:
        x = torch.from_numpy(pred).cuda()
    assert same(K.detections_to_boxes(x, 854, 480, inp, **kw), want)


def test_ties_and_nms_chains():
    pred, expect = tie_rows()
    kw = dict(confidence=0.25, nms=0.5, max_boxes=16)
    want = detect_decode_np(pred, 64, 64, 64, **kw)
    r = K.detections_to_boxes(torch.from_numpy(pred).cuda(), 64, 64, 64, **kw)
    assert same(r, want)
    assert r.index[0, :6].tolist() == expect and int(r.count[0]) == 6 and int(r.candidates[0]) == 8
    assert torch.isnan(r.boxes[0, 5, 5]) and not torch.isnan(r.boxes[0, :, :5]).any(), "the NaN class score in first place is the winner's score"


def crowd(n_rows=3000, seed=5):
    """prediction [2,n_rows,7] (C = 2): every second row of image 0 a person above the threshold with its own objectness, boxes on a jittered lattice of a
    416 input so that most have overlapping neighbours; image 1 has 40 persons."""
    g = np.random.default_rng(seed)
    p = np.zeros((2, n_rows, 7), F32)
    p[..., 0:2] = g.uniform(20, 396, size=(2, n_rows, 2))
    p[..., 2:4] = g.uniform(8, 30, size=(2, n_rows, 2))
    p[..., 4] = (g.permutation(2 * n_rows).reshape(2, n_rows) + 1) / F32(4 * n_rows)    # distinct, in (0, 0.5]
    p[0, ::2, 4] += F32(0.5)
    p[1, :40, 4] += F32(0.5)
    p[..., 5], p[..., 6] = 0.9, 0.2
    p[0, 1::8, 4] += F32(0.5)                                                            # ... and some other objects above the threshold
    p[0, 1::8, 5] = 0.1
    return p


def test_caps_cut_prefixes_and_report_the_uncapped_count():
    pred = crowd()
    x = torch.from_numpy(pred).cuda()
    kw = dict(confidence=0.5, nms=0.4)
    full = detect_decode_np(pred, 1280, 720, 416, max_boxes=4096, max_candidates=4096, **kw)
    assert full[2].tolist() == [1500, 40] and full[1][0] > 300, "more candidates than the default cap, more survivors than the default rows"
    assert same(K.detections_to_boxes(x, 1280, 720, 416, max_boxes=4096, max_candidates=4096, **kw), full), "the largest cap: 4,096 candidates in LDS"
    for mc, mb in ((1024, 32), (1024, 1024), (100, 100), (1499, 7), (1, 1), (2048, 300)):
        r = K.detections_to_boxes(x, 1280, 720, 416, max_boxes=mb, max_candidates=mc, **kw)
        assert same(r, detect_decode_np(pred, 1280, 720, 416, max_boxes=mb, max_candidates=mc, **kw)), (mc, mb)
        assert r.candidates.tolist() == [1500, 40], "the uncapped number"
        n = r.count.tolist()
        for b in range(2):
            assert 1 <= n[b] <= mb and bits(r.boxes[b, :n[b]]) == full[0][b, :n[b]].tobytes() and r.index[b, :n[b]].tolist() == full[3][b, :n[b]].tolist()
            assert not r.boxes[b, n[b]:].any() and (r.index[b, n[b]:] == -1).all()
        assert n[0] == mb or mc < 1500 or n[0] == full[1][0]


def test_images_are_independent_and_runs_repeat():
    fx = golden()
    heads, pred, w, h, inp = group(fx, "b")
    pred = np.concatenate((pred[:1], pred[:1] * 0, pred[1:]), axis=0)                  # an image without a person in second place
    pred[1, :, 4] = 0.9
    pred[1, :, 6] = 0.99                                                                # ... full of confident non-persons
    x = torch.from_numpy(pred).cuda()
    r = K.detections_to_boxes(x, w, h, inp, **KW)
    assert r.count.tolist() == [int(fx["b_ref_count"][0]), 0] + fx["b_ref_count"][1:].tolist() and r.candidates[1] == 0
    assert not r.boxes[1].any() and (r.index[1] == -1).all()
    for b in (0, 2, 3):
        assert bits(r.boxes[b]) == fx["b_ref_boxes"][b - (b > 1)].tobytes()
    for b in range(4):
        alone = K.detections_to_boxes(x[b:b + 1], w, h, inp, **KW)
        assert all(bits(a[0]) == bits(c[b]) for a, c in zip(alone, r)), b
    hs = [torch.from_numpy(hd).cuda() for hd in heads]
    first = K.yolo_heads_to_boxes(hs, w, h, inp, **KW)
    for _ in range(3):
        again = K.yolo_heads_to_boxes(hs, w, h, inp, **KW)
        assert all(bits(a) == bits(c) for a, c in zip(first, again))
    for b in range(3):
        alone = K.yolo_heads_to_boxes([t[b:b + 1] for t in hs], w, h, inp, **KW)
        assert all(bits(a[0]) == bits(c[b]) for a, c in zip(alone, first)), b
    empty = K.detections_to_boxes(x[:0], w, h, inp, **KW)
    assert tuple(empty.boxes.shape) == (0, 32, 6) and tuple(empty.count.shape) == (0,) and tuple(empty.index.shape) == (0, 32), "an empty batch"


def test_per_image_frames_and_clamping():
    fx = golden()
    heads, pred, w, h, inp = group(fx, "a")
    pred = pred.copy()
    pred[:, 0, :4] = (inp / 2, inp / 2, 3 * inp, 3 * inp)                              # a person larger than the input: clamped on all four sides
    pred[:, 0, 4:] = 0
    pred[:, 0, 4:6] = (0.999, 0.9)
    widths, heights = np.array([854, 1080, 640], F32), np.array([480, 1920, 640], F32)      # landscape, portrait, square
    want = detect_decode_np(pred, widths, heights, inp, **KW)
    for wv, hv in ((widths, heights), (torch.from_numpy(widths).cuda(), torch.from_numpy(heights).cuda()), (widths.tolist(), torch.from_numpy(heights))):
        r = K.detections_to_boxes(torch.from_numpy(pred).cuda(), wv, hv, inp, **KW)
        assert same(r, want)
    for b in range(3):
        assert r.index[b, 0] == 0 and r.boxes[b, 0, :4].tolist() == [0.0, 0.0, float(widths[b]), float(heights[b])]
        assert (r.boxes[b, :, 0] >= 0).all() and (r.boxes[b, :, 2] <= float(widths[b])).all() and (r.boxes[b, :, 3] <= float(heights[b])).all()
    hs = [torch.from_numpy(hd).cuda() for hd in heads]
    r = K.yolo_heads_to_boxes(hs, widths, heights, inp, **KW)
    close(r, detect_decode_np(heads, widths, heights, inp, form="heads", ft=F64, **KW), float(fx["b_ref_err_xy"]), float(fx["b_ref_err_score"]))


def test_boxes_go_into_the_heatmap_decode():
    fx = golden()
    heads, pred, w, h, inp = group(fx, "a")
    r = K.detections_to_boxes(torch.from_numpy(pred).cuda(), w, h, inp, **KW)
    n = int(r.count[0])
    hm = torch.rand((n, 17, 16, 12), device="cuda")
    kp = K.heatmaps_to_keypoints(hm, boxes=r.boxes[0, :n, :4], aspect=h / w)
    assert tuple(kp.shape) == (n, 17, 3) and torch.isfinite(kp).all()
    from tests.test_heatmap_cpu import heatmap_decode_np
    assert torch.equal(kp.cpu(), torch.from_numpy(heatmap_decode_np(hm.cpu().numpy(), boxes=fx["a_ref_boxes"][0, :n, :4], aspect=h / w)))
