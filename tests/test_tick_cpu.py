"""The whole video tick without a GPU: the synthetic scene and the composed restatement of tests/tick_ref.py held to the conditions tests/test_gpu_tick.py
relies on.  The chain of numpy restatements alone -- surface, letterbox, stand-in detector, decode, SORT, crop, stand-in pose network, heatmap decode,
One-Euro filter, overlay, encoder surface -- must find the planted joints within a bound DERIVED from the geometry, see every planted player and nothing else,
contain every feature the scene was built for, and leave the bound (or lose a detection) as soon as one side of a hand-off states its convention differently.

BOUND (tick_ref.bound) per axis and COCO joint: 0.75 heatmap cell -- half a cell from the argmax, a quarter from the refinement -- of the person's crop in
frame pixels, plus 1 px for the marker's rounding to a pixel and the chroma's 2 x 2 siting.  The keypoints the chain hands on are H36M (layout="h36m" is
coco_to_h36m of the COCO decode, and the pose network's joints are COCO's), so an H36M coordinate is held to BOUND times the row sum of |coefficients| of
the conversion, read off coco_h36m_np itself: 1 for the 13 copied joints, pelvis, neck and every x but the spine's; 5/3 for the spine's x, 7/3 for the
thorax's y and 3 for the head's y (= y_leye + y_reye - y_nose).  Observed when written: the worst ratio is 0.446 (1.49 px)."""
import numpy as np
import pytest

from tests import tick_ref as R
from tests.test_gpu_draw import round_trip_limit

F32 = np.float32


@pytest.fixture(scope="module")
def scene():
    return R.Scene()


@pytest.fixture(scope="module")
def chain(scene):
    """The 14 ticks through the restatements, min_hits = 0 (the demo's tracker)."""
    return R.run_np(scene, min_hits=0)


def evaluate(scene, run):
    """-> (worst |error| / bound over every tick, row and marked joint; the worst error in px; whether every planted player was detected, tracked and found in
    exactly one row in every tick; per tick the player of every row)."""
    worst, worst_px, seen_all, owners = 0.0, 0.0, True, []
    for t, o in enumerate(run):
        present = [p for p in range(3) if scene.present[t, p]]
        rows = []
        for k in range(o.track["person_count"]):
            p, ratio, err = R.owner_and_ratio(scene, t, o.kp_raw[k], o.scale[k])
            worst, worst_px = max(worst, ratio), max(worst_px, err)
            rows.append(p)
        owners.append(rows)
        seen_all = seen_all and sorted(o.index[0, :o.count[0]].tolist()) == [R.PLAYER_ROWS[p] for p in present] and sorted(rows) == present
    return worst, worst_px, seen_all, owners


def test_the_scene_is_what_its_docstring_says(scene):
    seen = np.concatenate((scene.markers_seen, scene.torsos_seen)).astype(int)
    painted = np.concatenate((scene.markers, scene.torsos)).astype(int)
    assert np.abs(seen - painted).max() <= max(int(v) for v in round_trip_limit("bt601", False).values()), "a flat patch comes back within the round trip's bound"
    d = np.abs(seen[:, None] - seen[None]).max(axis=-1) + 1000 * np.eye(20, dtype=int)
    assert d.min() >= 90 > R.TAU, "any two of the 20 colours are further apart than the pose network's window"
    for other in (0, 128 - 14, 128 + 14):                            # the crop's border, the background's and the letterbox canvas' greys
        assert np.abs(seen - other).max(axis=-1).min() >= R.TAU + R.DET_TOL, other
    assert scene.frames.shape == (R.TICKS, R.HF, R.WF, 3) and scene.surfaces.shape == (R.TICKS, R.SURFACE_ROWS, R.PITCH)
    assert (scene.surfaces[:, :, R.WF:] == R.PAD_BYTE).all() and (scene.surfaces[:, R.HF:R.CHROMA_ROW] == R.PAD_BYTE).all(), "the padding is marked"
    step = np.abs(np.diff(scene.coco, axis=0))
    assert 0 < step.max() <= 3.0, "at most 3 px per tick"
    # players 0 and 1 overlap, by less than the tracker's threshold, and neither's markers lie in the other's enlarged crop region
    for t in range(R.TICKS):
        a, b = scene.boxes[t, 0], scene.boxes[t, 1]
        w, h = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
        assert w > 0 and h > 0 and 0 < w * h / (2 * R.BOX_W * R.BOX_H - w * h) < 0.3
        for me, you in ((0, 1), (1, 0)):
            half = np.array([1.25 * R.BOX_W / 2, 1.25 * R.BOX_W / 2 * R.SIZE[1] / R.SIZE[0]])
            off = np.abs(scene.coco[t, you] - scene.centre[t, me]) - R.MARKER_R
            assert ((off > half + 1.0).any(axis=-1)).all(), "one player's markers in the other's crop would be that joint twice"
    assert (scene.boxes[:, 2, 2] > R.WF).all() and (scene.boxes[:, :2, 2] < R.WF).all(), "player 2 stands partly outside the right edge"
    for t in range(R.TICKS):
        assert np.nonzero(~scene.marked[t, 2])[0].tolist() == [7, 9] and scene.marked[t, 0].all(), "its left elbow and wrist have no marker"
        assert np.nonzero(~scene.h36m_marked[t, 2])[0].tolist() == [12, 13]
    a, b = R.ABSENT[1]
    assert b - a + 1 > R.MAX_AGE and a > 0 and b < R.TICKS - 1
    lay = R.LAYOUTS
    dist = np.sqrt(((lay[:, :, None] - lay[:, None]) ** 2).sum(-1)) + 1000 * np.eye(17)
    assert dist.min() > 2 * R.MARKER_R + 1, "no two discs of a player touch"
    assert np.abs(lay[0] - lay[1]).max() > 2 * R.bound((1.25 * R.BOX_W / 200,)), "players 0 and 1 differ by more than twice the bound in some joint"
    gain = scene.gain
    assert np.allclose(gain[[7, 8, 10]], [[5 / 3, 1], [1, 7 / 3], [1, 3]], atol=1e-6) and np.allclose(np.delete(gain, [7, 8, 10], axis=0), 1.0, atol=1e-6)


def test_ground_truth_is_recovered_by_the_reference_alone(scene, chain):
    worst, worst_px, seen_all, owners = evaluate(scene, chain)
    print(f"restatement chain against the plant: worst |error| / BOUND = {worst:.3f}, worst |error| = {worst_px:.2f} px")
    assert seen_all
    assert worst < 1.0, "BOUND is derived; a chain outside it needs larger markers or crops, never a larger bound"
    for t, o in enumerate(chain):                                    # the steadied keypoints stay with their player too
        for k, p in enumerate(owners[t]):
            assert R.owner_and_ratio(scene, t, o.kp[k], o.scale[k])[0] == p, (t, k)


def test_the_tracker_sees_every_planted_player(scene, chain):
    _, _, seen_all, owners = evaluate(scene, chain)
    assert seen_all
    ids = {}
    for t, o in enumerate(chain):
        present = [p for p in range(3) if scene.present[t, p]]
        r = o.track
        assert o.count[0] == r["count"] == r["person_count"] == len(present), t
        assert o.index[0, :o.count[0]].tolist() == [R.PLAYER_ROWS[p] for p in present], "the planted rows by objectness, and no decoy"
        assert o.valid.tolist() == [k < len(present) for k in range(R.NUM_PERSON)], t
        for k, p in enumerate(owners[t]):                            # persons: oldest first; ids: newest first
            box = scene.boxes[t, p].copy()
            box[2] = min(box[2], R.WF)
            assert np.abs(o.persons[k] - box).max() < 8.0, (t, k, "the row's box is its player's, up to the Kalman filter's lag")
            ids.setdefault(p, []).append((t, int(r["ids"][r["count"] - 1 - k])))
    assert len({i for _, i in ids[0]}) == 1 and len({i for _, i in ids[2]}) == 1, "one id while present"
    before, after = {i for t, i in ids[1] if t < R.ABSENT[1][0]}, {i for t, i in ids[1] if t > R.ABSENT[1][1]}
    assert len(before) == 1 and len(after) == 1 and before != after, "the returning player is a new track"
    assert len({i for v in ids.values() for _, i in v}) == 4


def test_every_scene_feature_occurs(scene, chain):
    for t, o in enumerate(chain):
        dup = o.pred[0, R.DUPLICATE_ROW]
        assert dup[4] > R.CONFIDENCE and dup[5] > dup[6] and o.candidates[0] == o.count[0] + 1, "the duplicate is a person above the confidence: NMS drops it"
        assert o.pred[0, R.LOW_ROW, 4] < R.CONFIDENCE and o.pred[0, R.OTHER_ROW, 4] > R.CONFIDENCE and o.pred[0, R.OTHER_ROW, 6] > o.pred[0, R.OTHER_ROW, 5]
        k = [k for k in range(o.track["person_count"]) if R.owner_and_ratio(scene, t, o.kp_raw[k], o.scale[k])[0] == 2][0]
        m = scene.h36m_marked[t, 2]
        assert (o.kp_raw[k][~m, 2] < R.MIN_SCORE).all() and (~m).sum() == 2, "the edge player's marker-less joints score below min_score"
        for kk in range(o.track["person_count"]):
            p = R.owner_and_ratio(scene, t, o.kp_raw[kk], o.scale[kk])[0]
            assert (o.kp_raw[kk][scene.h36m_marked[t, p], 2] > R.MIN_SCORE).all(), "every marked joint scores above it"
        if t:                                                        # ... and the filter holds them at its estimate while the marked ones move
            assert not np.array_equal(o.kp[k][m, :2], o.kp_raw[k][m, :2])
    gone = [t for t, o in enumerate(chain) if o.count[0] == 2]
    assert gone == list(range(R.ABSENT[1][0], R.ABSENT[1][1] + 1)) and len(gone) > R.MAX_AGE
    assert any(o.track["born"].any() for o in chain[1:]), "a birth after the first tick"
    painted = [int((o.painted != o.frame).any(axis=-1).sum()) for o in chain]
    assert min(painted) > 500, "skeletons are drawn in every tick"


def test_default_min_hits_emits_the_returning_player_late_and_unborn(scene):
    run = R.run_np(scene, min_hits=3)
    back = R.ABSENT[1][1] + 1
    counts = [o.track["count"] for o in run]
    assert counts[:back] == [o.track["count"] for o in R.run_np(scene, min_hits=0, ticks=back)], "ticks <= min_hits emit from the first tick"
    assert counts[back:back + 3] == [2, 2, 2] and counts[back + 3] == 3 and not run[back + 3].track["born"].any(), "three hits first, then a row with born = 0"
    worst, _, _, _ = evaluate(scene, run[:back])
    assert worst < 1.0


def _shifted_boxes(res):
    """detect_decode_np's result as a detector would give it that forgot the letterbox's vertical offset on the way back to frame pixels."""
    boxes, count, cands, index = res
    new_w, new_h, pad_x, pad_y = R.plan_np(R.WF, R.HF, R.INP, R.INP)
    boxes = boxes.copy()
    for b in range(len(count)):
        boxes[b, :count[b], 1] += F32(pad_y * R.HF / new_h)
        boxes[b, :count[b], 3] += F32(pad_y * R.HF / new_h)
    return boxes, count, cands, index


def _reversed_rows(frame, persons):
    out, c, s = R.op_crop(frame, persons[::-1])
    return out, c[::-1], s[::-1]


WRONG = {
    "center_and_scale_swapped": dict(decode=lambda hm, c, s: R.op_decode(hm, s, c)),
    "pixel_std_160": dict(crop=lambda f, p: (lambda out, c, s: (out, c, s * F32(200.0 / 160.0)))(*R.op_crop(f, p))),
    "letterbox_offset_dropped": dict(detect=lambda pred: _shifted_boxes(R.op_detect(pred))),
    "swap_rb_flipped": dict(crop=lambda f, p: R.crop_persons_np(f, p, size=R.SIZE, swap_rb=False)),
    "persons_reversed_before_the_crop": dict(crop=_reversed_rows),
}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_a_wrong_convention_violates_the_bound(name, scene):
    """Each hand-off convention stated differently on one side, applied by wrapping a restatement: the chain leaves BOUND or loses a player (two ticks are
    enough: nothing here needs history)."""
    run = R.run_np(scene, min_hits=0, ops=dict(R.OPS, **WRONG[name]), ticks=2)
    worst, worst_px, seen_all, _ = evaluate(scene, run)
    print(f"{name}: worst |error| / BOUND = {worst:.2f} ({worst_px:.1f} px), every player seen: {seen_all}")
    assert worst > 1.0 or not seen_all


def test_the_encoders_surface_decodes_to_the_painted_frame(scene, chain):
    """yuv_to_bgr of the encoder's planes against the painted frame, within the bound tests/test_gpu_draw.py derives for a flat colour.  That bound holds where
    the quad's mean IS the pixel's colour as far as the chroma goes: on quads of one colour and on grey quads (whose chroma is neutral whatever their luma);
    those are most of the frame, and the inside of every torso, marker and bone."""
    from tests.test_yuv_cpu import yuv_to_bgr_np
    limit = round_trip_limit("bt601", False)
    for o in chain[::6]:
        back = yuv_to_bgr_np(o.enc_y, o.enc_uv).astype(int)
        p = o.painted.astype(int)
        q = p.reshape(R.HF // 2, 2, R.WF // 2, 2, 3)
        flat = (q == q[:, :1, :, :1]).all(axis=(1, 3, 4))
        grey = ((q[..., 0] == q[..., 1]) & (q[..., 1] == q[..., 2])).all(axis=(1, 3))
        ok = np.repeat(np.repeat(flat | grey, 2, axis=0), 2, axis=1)
        assert ok.mean() > 0.95 and (ok & (p != o.frame).any(axis=-1)).sum() > 200, "most of the frame, and painted pixels among them"
        err = np.abs(back - p)[ok].max(axis=0)
        for c, name in enumerate("BGR"):
            assert err[c] <= int(limit[name]), (name, err)
