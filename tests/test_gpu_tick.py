"""The whole video tick on the GPU, decoder surface in, encoder surface out ("the whole tick"): the chain

    nv12_to_bgr -> letterbox_frames -> detections_to_boxes -> SortTracker.update -> crop_persons -> heatmaps_to_keypoints(layout="h36m")
    -> OneEuroFilter.push -> TrackedLifter.push -> draw_poses(surface=...)

written out as a user writes it (``tick`` below), on the synthetic scene and the stand-in networks of tests/tick_ref.py, 14 ticks, model n_layers = 1,
n_frames = 27, fp32.  Every op has a test file of its own against its restatement; what is held HERE is that the ops fit together:

  stage by stage   in every tick each stage's device output against that stage's restatement APPLIED TO WHAT THE DEVICE PRODUCED in the stage before, at the
                   bar of the stage's own test file: bits (np.array_equal) for the surface conversion, the letterbox (its cubic bound is the restatement's,
                   against exact convolution, on the CPU; device against restatement is bits in tests/test_gpu_letterbox.py too), the detector decode
                   (``same`` of tests/test_gpu_detect.py), the crop, the heatmap decode, the filter, the overlay and the encoder's planes; ``check_tick`` of
                   tests/test_gpu_track.py for the tracker (ids, slots, births, counts and order exact, boxes within one fp32 ulp, fp64 state within its
                   bar); torch.equal for the lifter against a plain StreamLifter driven from the read-back TrackResult with the same keypoints.
  end to end       the decoded keypoints within tick_ref.bound (derived, tests/test_tick_cpu.py) of the planted joints; row k of t.persons, r.inputs, the
                   decoded and the steadied keypoints, out.ids and -- through the stage check -- out.poses belongs to one planted player; out.valid is true
                   exactly below person_count; ids as tests/test_tick_cpu.py states them.
  nothing else     the source surface and the BGR frame are unchanged after the tick; the frame and the encoder's planes are views of larger sentinel-filled
                   buffers behind padded pitches, and every byte outside the payload keeps the sentinel.
  repeatable       two runs give the same bytes at every stage.
  no host sync     one steady-state tick under torch.cuda.set_sync_debug_mode("error"), with the control and the vacuous-pass skip of tests/test_gpu_tracked.py.
  two streams      two different scenes through the batched forms of every op; stream 0 has the bytes of the single-stream run.
  min_hits         0 (the demo's) and the default 3, where the returning player's row appears three ticks late with born = 0.

Nothing here provokes a fault; no test looks at a kernel's assembly."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import smooth_ref, tick_ref as R
from tests.gpu_util import make_pair
from tests.test_gpu_detect import same as detect_same
from tests.test_gpu_draw import SENTINEL, only_payload_changed, pitched
from tests.test_gpu_track import check_tick
from tests.test_track_cpu import tracker_state_np

pytestmark = pytest.mark.gpu

_SHARED = {}


def scene(which=0):
    key = ("scene", which)
    if key not in _SHARED:
        _SHARED[key] = R.Scene() if which == 0 else R.Scene(seed=1, shift=(-40.0, 30.0))
    return _SHARED[key]


def model():
    if "model" not in _SHARED:
        _SHARED["model"] = make_pair(1, 27, "fp32")[1].eval()
    return _SHARED["model"]


def host(t):
    return t.detach().cpu().numpy()


class Pipeline:
    """What a user builds once for ``streams`` video streams: the tracker, the filter, the lifter, the frame's size on the device (a host number would be
    uploaded in every tick, which synchronises) and the buffers the frame and the encoder's planes are written into."""

    def __init__(self, scenes, min_hits=0):
        import kasportsformer_amd as K
        B = self.streams = len(scenes)
        self.nets = [R.StandIns(s, "cuda") for s in scenes]
        self.trk = K.SortTracker(streams=B, slots=R.SLOTS, max_age=R.MAX_AGE, min_hits=min_hits, num_person=R.NUM_PERSON)
        self.f2 = K.OneEuroFilter(streams=B, track_slots=R.SLOTS, rows="persons", num_person=R.NUM_PERSON, min_score=R.MIN_SCORE)
        self.lifter = K.TrackedLifter(model(), R.WF, R.HF, streams=B, track_slots=R.SLOTS, rows="persons", num_person=R.NUM_PERSON)
        self.fw, self.fh = torch.full((B,), float(R.WF), device="cuda"), torch.full((B,), float(R.HF), device="cuda")
        self.frame_index = torch.arange(B, device="cuda", dtype=torch.int32).repeat_interleave(R.NUM_PERSON)
        ch, cw = (R.HF + 1) // 2, (R.WF + 1) // 2
        fp, yp, cp = 3 * R.WF + 24, R.WF + 16, 2 * cw + 8
        self.frame_buf, frame = pitched((B, R.HF, R.WF), fp, R.HF * fp + 16, 0, SENTINEL, 3)
        self.y_buf, y = pitched((B, R.HF, R.WF), yp, R.HF * yp + 16, 0, SENTINEL, 1)
        self.uv_buf, uv = pitched((B, ch, cw), cp, ch * cp + 8, 0, SENTINEL, 2)
        one = B == 1
        self.frame_out, self.enc_y, self.enc_uv = (frame[0] if one else frame), (y[0, ..., 0] if one else y[..., 0]), (uv[0] if one else uv)
        self.views = ((self.frame_buf, frame), (self.y_buf, y), (self.uv_buf, uv))

    def detector(self, inputs, n):
        return torch.cat([net.detector(inputs[b:b + 1], n) for b, net in enumerate(self.nets)])

    def pose_network(self, inputs):
        return self.nets[0].pose_network(inputs)                 # the marker colours are every scene's


def tick(p, surface, n):
    """One tick of one stream, as INTEGRATION.md writes it; ``n`` is the tick's number, which only the stand-in detector needs."""
    import kasportsformer_amd as K
    frame = K.nv12_to_bgr(surface, R.HF, R.WF, chroma_row=R.CHROMA_ROW, out=p.frame_out)                   # convert
    lb = K.letterbox_frames(frame, inp_dim=R.INP)                                                          # letterbox
    pred = p.detector(lb.inputs, n)
    d = K.detections_to_boxes(pred, p.fw, p.fh, inp_dim=R.INP, confidence=R.CONFIDENCE)                    # detect
    t = p.trk.update(d.boxes, d.count)                                                                     # track
    r = K.crop_persons(frame, t.persons[0], size=R.SIZE)                                                   # crop
    hm = p.pose_network(r.inputs)
    kp_raw = K.heatmaps_to_keypoints(hm, r.center, r.scale, layout="h36m")                                 # decode
    kp = p.f2.push(kp_raw, t)                                                                              # steady
    out = p.lifter.push(kp, t)                                                                             # lift
    enc = K.draw_poses(frame, kp, out.valid[0], min_score=R.MIN_SCORE, out=False, surface=(p.enc_y, p.enc_uv))      # draw + convert
    return SimpleNamespace(frame=frame, lb=lb, pred=pred, d=d, t=t, r=r, hm=hm, kp_raw=kp_raw, kp=kp, out=out, enc=enc)


def tick_batched(p, surfaces, n):
    """The same tick for ``p.streams`` streams at once: every op in its batched form, nothing read back."""
    import kasportsformer_amd as K
    B, P = p.streams, R.NUM_PERSON
    frames = K.nv12_to_bgr(surfaces, R.HF, R.WF, chroma_row=R.CHROMA_ROW, out=p.frame_out)                 # [B,Hf,Wf,3]
    lb = K.letterbox_frames(frames, inp_dim=R.INP)
    pred = p.detector(lb.inputs, n)
    d = K.detections_to_boxes(pred, p.fw, p.fh, inp_dim=R.INP, confidence=R.CONFIDENCE)
    t = p.trk.update(d.boxes, d.count)
    r = K.crop_persons(frames, t.persons.view(B * P, 4), size=R.SIZE, frame_index=p.frame_index)
    hm = p.pose_network(r.inputs)
    kp_raw = K.heatmaps_to_keypoints(hm, r.center, r.scale, layout="h36m")                                 # [B*P,17,3]
    kp = p.f2.push(kp_raw, t)
    out = p.lifter.push(kp, t)
    enc = K.draw_poses(frames, kp.view(B, P, 17, 3), out.valid, min_score=R.MIN_SCORE, out=False, surface=(p.enc_y, p.enc_uv))
    return SimpleNamespace(frame=frames, lb=lb, pred=pred, d=d, t=t, r=r, hm=hm, kp_raw=kp_raw, kp=kp, out=out, enc=enc)


def record(p, o, stream=0):
    """Everything a tick produced for one stream, on the host."""
    B, P = p.streams, R.NUM_PERSON
    rows = slice(stream * P, (stream + 1) * P)
    pick = (lambda a: host(a)[stream]) if B > 1 else host
    rec = dict(frame=pick(o.frame), lb=host(o.lb.inputs)[stream], pred=host(o.pred)[stream], hm=host(o.hm)[rows], inputs=host(o.r.inputs)[rows],
               center=host(o.r.center)[rows], scale=host(o.r.scale)[rows], kp_raw=host(o.kp_raw)[rows], kp=host(o.kp)[rows], enc_y=pick(o.enc.y), enc_uv=pick(o.enc.uv))
    rec.update({"d_" + k: host(getattr(o.d, k))[stream] for k in o.d._fields})
    rec.update({"t_" + k: host(getattr(o.t, k))[stream] for k in o.t._fields})
    rec.update({"out_" + k: host(getattr(o.out, k))[stream] for k in o.out._fields})
    return rec


def run(min_hits=0, fresh=False):
    """The 14 ticks of scene 0 through ``tick`` -> per tick the record, the tracker's state and what the write checks saw.  Shared by the tests below."""
    key = ("run", min_hits)
    if key in _SHARED and not fresh:
        return _SHARED[key]
    import kasportsformer_amd as K
    sc = scene()
    p = Pipeline([sc], min_hits)
    surfaces = torch.from_numpy(sc.surfaces).cuda()
    keep = surfaces.clone()
    before = [b.clone() for b, _ in p.views]
    ticks = []
    for n in range(R.TICKS):
        o = tick(p, surfaces[n], n)
        assert o.frame.data_ptr() == p.frame_out.data_ptr() and o.enc.y.data_ptr() == p.enc_y.data_ptr() and o.enc.uv.data_ptr() == p.enc_uv.data_ptr() and o.enc.frame is None
        rec = record(p, o)
        s = p.trk.state()
        rec["state"] = {k: host(getattr(s, k))[0] for k in s._fields}
        rec["detect_same"] = detect_same(o.d, R.op_detect(host(o.pred)))
        rec["lb_meta"] = (o.lb.width, o.lb.height, o.lb.size, o.lb.offset)
        rec["by_valid"] = host(K.draw_poses(o.frame, o.kp, o.out.valid[0]).frame)       # no min_score: only `valid` decides which rows are drawn
        rec["padding_kept"] = all(only_payload_changed(b, v, k) for (b, v), k in zip(p.views, before))
        ticks.append(rec)
    torch.cuda.synchronize()
    res = dict(ticks=ticks, surfaces_kept=torch.equal(surfaces, keep), pipeline=p)
    if not fresh:
        _SHARED[key] = res
    return res


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("min_hits", [0, 3])
def test_every_stage_follows_its_restatement_on_the_devices_own_input(min_hits):
    import kasportsformer_amd as K
    sc = scene()
    ticks = run(min_hits)["ticks"]
    trk = R.new_tracker(slots=R.SLOTS, max_age=R.MAX_AGE, min_hits=min_hits, num_person=R.NUM_PERSON)
    f2 = smooth_ref.new_state(R.SLOTS, 17, 2)
    plain = K.StreamLifter(model(), R.WF, R.HF, slots=R.SLOTS)
    holder, pushed, unused = {}, 0, 0
    for n, g in enumerate(ticks):
        assert np.array_equal(g["frame"], R.op_frame(sc.surfaces[n])), (n, "surface -> BGR")
        assert bits_equal(g["lb"][None], R.op_letterbox(g["frame"])), (n, "letterbox")
        new_w, new_h, pad_x, pad_y = R.plan_np(R.WF, R.HF, R.INP, R.INP)
        assert g["lb_meta"] == (R.WF, R.HF, (new_w, new_h), (pad_x, pad_y)), n
        assert g["detect_same"], (n, "detector decode")
        want = R.op_track(trk, g["d_boxes"], g["d_count"])
        want["state"] = tracker_state_np(trk)
        got = {k[2:]: v for k, v in g.items() if k.startswith("t_")}
        got["state"] = g["state"]
        check_tick(got, want, ("tracker", n))
        inputs, center, scale = R.op_crop(g["frame"], g["t_persons"])
        assert bits_equal(g["inputs"], inputs) and bits_equal(g["center"], center) and bits_equal(g["scale"], scale), (n, "crop")
        assert bits_equal(g["kp_raw"], R.op_decode(g["hm"], g["center"], g["scale"])), (n, "heatmap decode")
        arrays = {k: g["t_" + k][None] for k in ("ids", "slot", "born")}
        arrays["count"] = np.array([g["t_count"]], np.int32)
        kp, row_slot, _, _ = R.op_filter(f2, g["kp_raw"], arrays, n)
        assert bits_equal(g["kp"], kp), (n, "One-Euro filter")
        assert g["out_valid"].tolist() == (row_slot >= 0).tolist() == [k < g["t_person_count"] for k in range(R.NUM_PERSON)], (n, "valid")
        # the lifter: a plain StreamLifter driven from the read-back TrackResult with the same keypoints
        c, kpd = int(g["t_count"]), torch.from_numpy(g["kp"]).cuda()
        for k in range(R.NUM_PERSON):
            if k >= c:
                assert not g["out_valid"][k] and not g["out_poses"][k].any() and g["out_ids"][k] == 0 and g["out_frames"][k] == 0, (n, k)
                continue
            row = c - 1 - k
            i, s, born = int(g["t_ids"][row]), int(g["t_slot"][row]), int(g["t_born"][row])
            if holder.get(s) != i or born:
                plain.reset(slots=[s])
                holder[s] = i
            pose = plain.push(kpd[k:k + 1], slots=[s])
            pushed += 1
            assert g["out_valid"][k] and g["out_ids"][k] == i and g["out_frames"][k] == int(plain.counts[s]), (n, k)
            assert torch.equal(torch.from_numpy(g["out_poses"][k]).cuda(), pose[0]), (n, k, "lifter")
        painted = R.op_draw(g["frame"], g["kp"], g["out_valid"])
        wy, wuv = R.op_surface(painted)
        assert np.array_equal(g["enc_y"], wy) and np.array_equal(g["enc_uv"], wuv), (n, "overlay and encoder surface")
        assert (painted != g["frame"]).any(), n
        # ... and without min_score, where `valid` alone keeps an unused row (all its joints at the frame's corner) from being drawn
        by_valid = R.draw_poses_np(g["frame"][None], g["kp"][None], g["out_valid"][None], colors=R.wheel(16), boxed=True)[0]
        assert np.array_equal(g["by_valid"], by_valid), (n, "valid against what is drawn")
        if not g["out_valid"].all():
            unused += 1
            assert not np.array_equal(by_valid, R.draw_poses_np(g["frame"][None], g["kp"][None], None, colors=R.wheel(16), boxed=True)[0]), n
    assert pushed >= 2 * R.TICKS and unused >= 4, "ticks with a row that only `valid` keeps from being drawn"


@pytest.mark.parametrize("min_hits", [0, 3])
def test_end_to_end_against_the_plant(min_hits):
    sc = scene()
    ticks = run(min_hits)["ticks"]
    worst, worst_px, owner_of_id, ids_of = 0.0, 0.0, {}, {0: set(), 1: set(), 2: set()}
    mean_rgb, std_rgb = np.array(R.MEAN[::-1], np.float32), np.array(R.STD[::-1], np.float32)
    for n, g in enumerate(ticks):
        pc, c = int(g["t_person_count"]), int(g["t_count"])
        present = [p for p in range(3) if sc.present[n, p]]
        assert g["d_index"][:g["d_count"]].tolist() == [R.PLAYER_ROWS[p] for p in present] and g["d_candidates"] == g["d_count"] + 1, (n, "every player, no decoy")
        assert g["out_valid"].tolist() == [k < pc for k in range(R.NUM_PERSON)], n
        owners = []
        for k in range(pc):
            p, ratio, err = R.owner_and_ratio(sc, n, g["kp_raw"][k], g["scale"][k])
            print(f"min_hits {min_hits} tick {n} row {k}: player {p}, worst |error| {err:.2f} px = {ratio:.3f} of BOUND")
            assert ratio < 1.0, (n, k, p, ratio, err)
            worst, worst_px = max(worst, ratio), max(worst_px, err)
            owners.append(p)
            box = sc.boxes[n, p].copy()
            box[2] = min(box[2], R.WF)
            assert np.abs(g["t_persons"][k] - box).max() < 8.0, (n, k, "t.persons")
            centre = (g["inputs"][k][:, R.SIZE[1] // 2, R.SIZE[0] // 2] * std_rgb + mean_rgb) * 255.0
            assert np.abs(centre - sc.torsos_seen[p][::-1]).max() <= R.DET_TOL, (n, k, "r.inputs: the crop's centre is the player's torso")
            assert R.owner_and_ratio(sc, n, g["kp"][k], g["scale"][k])[0] == p, (n, k, "the filter's output")
            i = int(g["out_ids"][k])
            assert i == int(g["t_ids"][c - 1 - k]) and owner_of_id.setdefault(i, p) == p, (n, k, "out.ids")
            ids_of[p].add(i)
            m = sc.h36m_marked[n, p]
            assert (g["kp_raw"][k][m, 2] > R.MIN_SCORE).all() and (g["kp_raw"][k][~m, 2] < R.MIN_SCORE).all(), (n, k, "scores")
        assert len(set(owners)) == len(owners) and (min_hits or sorted(owners) == present), n
    print(f"min_hits {min_hits}: worst keypoint error against the plant {worst_px:.2f} px = {worst:.3f} of BOUND")
    assert len(ids_of[0]) == 1 and len(ids_of[2]) == 1, "one id while present"
    back = R.ABSENT[1][1] + 1
    if min_hits == 0:
        assert len(ids_of[1]) == 2, "the returning player is a new track"
        assert ticks[back]["t_born"][0] == 1 and ticks[back]["out_frames"][2] == 1
    else:
        late = ticks[back + 3]
        assert [int(g["t_count"]) for g in ticks[back:back + 3]] == [2, 2, 2] and late["t_count"] == 3 and not late["t_born"].any(), "three hits first"
        assert late["out_valid"].all() and late["out_frames"].tolist() == [back + 4, back + 4, 1], "born = 0: only the owner table starts the history"


def test_nothing_else_is_written():
    res = run(0)
    assert res["surfaces_kept"], "the source surfaces are only read"
    assert all(g["padding_kept"] for g in res["ticks"]), "every byte outside the frame's and the planes' payload keeps the sentinel"
    sc, p = scene(), Pipeline([scene()], 0)
    surface = torch.from_numpy(sc.surfaces[0]).cuda()
    o = tick(p, surface, 0)
    frame_after = host(o.frame)
    assert np.array_equal(frame_after, R.op_frame(sc.surfaces[0])), "the BGR frame is as the conversion left it after the whole tick (out=False paints nothing)"
    assert (host(p.frame_buf) == SENTINEL).sum() >= 24 * R.HF and (host(p.y_buf) == SENTINEL).sum() >= 16 * R.HF


def test_two_runs_give_the_same_bytes_at_every_stage():
    a, b = run(0)["ticks"], run(0, fresh=True)["ticks"]
    for n, (u, v) in enumerate(zip(a, b)):
        for k in u:
            if isinstance(u[k], np.ndarray):
                assert bits_equal(u[k], v[k]), (n, k)
            elif k == "state":
                assert all(bits_equal(u[k][f], v[k][f]) for f in u[k]), (n, k)


def test_a_steady_state_tick_does_not_synchronise_with_the_host():
    sc = scene()
    p = Pipeline([sc], 0)
    surfaces = torch.from_numpy(sc.surfaces[:3]).cuda()
    tick(p, surfaces[0], 0)                                                     # warm-up: code objects, workspaces, the overlay's tables
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    raised, ok = False, False
    o = tick(p, surfaces[1], 1)
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:                                                                    # the control: the read-back a caller needed before
            o.t.ids.cpu()
        except RuntimeError:
            raised = True
        if raised:
            o = tick(p, surfaces[2], 2)
            ok = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not raised:
        pytest.skip("this torch build does not raise on a device-to-host copy under set_sync_debug_mode('error'): the check would pass vacuously")
    assert ok and bool(o.out.valid.all()) and np.array_equal(host(o.frame), R.op_frame(sc.surfaces[2]))


def test_two_streams_through_the_batched_forms():
    scenes = [scene(0), scene(1)]
    p = Pipeline(scenes, 0)
    surfaces = torch.from_numpy(np.stack([s.surfaces for s in scenes], axis=1)).cuda()              # [T,2,rows,pitch]
    before = [b.clone() for b, _ in p.views]
    alone = run(0)["ticks"]
    worst = 0.0
    for n in range(R.TICKS):
        o = tick_batched(p, surfaces[n], n)
        g0, g1 = record(p, o, 0), record(p, o, 1)
        for k, v in g0.items():
            assert bits_equal(v, alone[n][k]), (n, k, "stream 0 of the batch has the bytes of the stream alone")
        assert np.array_equal(g1["frame"], R.op_frame(scenes[1].surfaces[n])) and not np.array_equal(g1["frame"], g0["frame"])
        for k in range(int(g1["t_person_count"])):                              # the other scene is found where it was planted
            player, ratio, err = R.owner_and_ratio(scenes[1], n, g1["kp_raw"][k], g1["scale"][k])
            assert ratio < 1.0, (n, k, player, ratio, err)
            worst = max(worst, ratio)
        assert g1["out_valid"].tolist() == [k < g1["t_person_count"] for k in range(R.NUM_PERSON)] and g1["t_person_count"] == scenes[1].present[n].sum()
        painted = R.op_draw(g1["frame"], g1["kp"], g1["out_valid"])
        wy, wuv = R.op_surface(painted)
        assert np.array_equal(g1["enc_y"], wy) and np.array_equal(g1["enc_uv"], wuv), n
    assert all(only_payload_changed(b, v, k) for (b, v), k in zip(p.views, before))
    print(f"stream 1: worst keypoint error {worst:.3f} of BOUND")
