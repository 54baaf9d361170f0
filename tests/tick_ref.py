"""Shared by tests/test_tick_cpu.py and tests/test_gpu_tick.py (not a test): a synthetic scene for the whole video tick of INTEGRATION.md -- decoder surface in,
encoder surface out --, two stand-in networks, and ``tick_np``, the chain of the EXISTING numpy restatements of every op (imported, never copied).

The scene: 14 ticks of a 360 x 640 BGR frame (grey noise 128 +- 12) with three players.  Each has a 60 x 90 box, a flat torso rectangle of its own colour and
one disc of radius ``MARKER_R`` per COCO joint that lies inside the frame, each joint in its own colour.  The pose network's joints are COCO's, so the markers
are: ``heatmaps_to_keypoints(layout="h36m")`` is ``coco_to_h36m`` of the COCO decode, and the planted H36M joints are ``coco_h36m_np`` of the planted COCO
joints (13 copies, and pelvis, spine, thorax, head as linear combinations).  Player 0 walks right; player 1 walks with it, its box overlapping player 0's in
a 2 x 10 pixel corner (IoU 0.002 > 0, below the tracker's 0.3 and NMS's 0.4) and free of either's markers, leaves for ticks 5..8 (longer than max_age = 1) and
comes back; player 2 stands at the right edge with its box reaching 9 pixels outside, so its left elbow and wrist have no marker.  The frame reaches the
device as an NV12 surface behind a pitch of 704 with the chroma plane at row 368 (``bgr_to_nv12_np``); padding bytes hold 0x5A.

The stand-ins are plain torch expressions that run on either device, launch no kernel of this project, read nothing back and are functions of the pixels the
stage before produced.  *Detector*: row 1 + 3 p of a [1,16,85] prediction holds player p's planted box mapped into the letterbox by ``plan_np``; its person
score (class 0) is 0.95 iff ``lb.inputs`` at the mapped box centre is within ``DET_TOL`` grey levels of the player's torso colour, else 0, and its class-1
score is always 0.5 -- so a row whose pixel does not match is another class's and is dropped (an all-zero class row would still count as class 0).  Decoys:
row 2 repeats player 0's box two pixels off with a lower objectness (NMS must drop it), row 10 is a person below the confidence, row 12 a confident
non-person.  *Pose network*: the crop is de-normalised (plane k holds frame channel 2 - k, normalised with mean / std [2 - k]: the demo's mix-up, restated
here from crop_persons' docstring), every pixel scores ``clamp(1 - max_c |pixel - marker_j| / TAU, 0, 1)`` against each marker colour and heatmap j is the
7 x 7 mean of that at stride 4, padding 3: cell i is centred on crop pixel 4 i, the position the decode maps heatmap coordinate i to.  With
``MARKER_R = 3`` and a 9 x 9 mean the chain stayed inside BOUND but the marked joints scored 0.21 .. 0.26, below ``MIN_SCORE``: the markers were enlarged and the
window narrowed (scores 0.50 .. 0.83), the bound was not touched.

Colours are compared with what a flat patch becomes through ``nv12_to_bgr_np(bgr_to_nv12_np(.))``, not with the painted values."""
from types import SimpleNamespace

import numpy as np
import torch

from tests import smooth_ref
from tests.test_coco_world_cpu import coco_h36m_np
from tests.test_crop_cpu import crop_persons_np
from tests.test_detect_cpu import detect_decode_np
from tests.test_draw_cpu import bgr_to_nv12_np, draw_poses_np, wheel
from tests.test_heatmap_cpu import heatmap_decode_np
from tests.test_letterbox_cpu import letterbox_np, plan_np
from tests.test_track_cpu import new_tracker, sort_update_np
from tests.test_yuv_cpu import nv12_to_bgr_np

F32, F64 = np.float32, np.float64
HF, WF, TICKS = 360, 640, 14
PITCH, CHROMA_ROW, SURFACE_ROWS, PAD_BYTE = 704, 368, 368 + 180, 0x5A
INP = 416
CONFIDENCE = 0.30
SIZE = (96, 128)                               # the crop's (width, height)
HM_W, HM_H = SIZE[0] // 4, SIZE[1] // 4
NUM_PERSON, SLOTS, MAX_AGE = 3, 8, 1
MIN_SCORE = 0.3
BOX_W, BOX_H = 60.0, 90.0
MARKER_R = 4
TAU, DET_TOL = 48.0, 12.0
N_ROWS, PLAYER_ROWS, DUPLICATE_ROW, LOW_ROW, OTHER_ROW = 16, (1, 4, 7), 2, 10, 12
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ABSENT = {1: (5, 8)}                           # player 1 is away for ticks 5..8
FILTER = smooth_ref.params(min_score=MIN_SCORE)

# COCO joints in box coordinates (x from the box's centre line, y from its top): nose, eyes, ears, shoulders, elbows, wrists, hips, knees, ankles; left = +x
LAYOUT = np.array([(0, 14), (5, 6), (-5, 6), (14, 12), (-14, 12), (13, 26), (-13, 26), (22, 38), (-22, 38), (26, 50), (-26, 50), (9, 56), (-9, 56),
                   (11, 69), (-11, 69), (12, 83), (-12, 83)], F64)
POSE_1 = {9: (27, 29), 10: (-27, 29), 15: (4, 83)}         # player 1 raises both wrists and pulls its left ankle in: a row permutation between two players
LAYOUTS = np.stack([LAYOUT, LAYOUT, LAYOUT])                #   must show, so no two players may look alike relative to their boxes (player 2's box is clamped)
for _j, _xy in POSE_1.items():
    LAYOUTS[1, _j] = _xy
TORSO = (-12, 22, 12, 62)                      # x0, y0, x1, y1 (inclusive) in the same coordinates
START = np.array([(150.0, 120.0), (150.0 + 58.0, 120.0 + 80.0), (619.0, 180.0)])
VELOCITY = np.array([(2.0, 0.5), (2.0, 0.5), (0.0, 1.0)])


def palette():
    """20 painted colours (B, G, R), a fixed choice from {30, 128, 226}^3 without grey (the background, the letterbox's canvas) and without the darkest (the
    crop's border is 0): any two differ by at least 98 in some channel.  -> (markers [17,3], torsos [3,3]) uint8."""
    grid = [(b, g, r) for b in (30, 128, 226) for g in (30, 128, 226) for r in (30, 128, 226) if (b, g, r) not in ((128, 128, 128), (30, 30, 30))]
    order = np.random.default_rng(7).permutation(len(grid))
    c = np.array([grid[i] for i in order], np.uint8)
    return c[:17], c[17:20]


def make_surface(frame):
    """BGR frame [HF,WF,3] -> the pitched NV12 surface [SURFACE_ROWS,PITCH] uint8 a decoder would hand over."""
    y, uv = bgr_to_nv12_np(frame)
    s = np.full((SURFACE_ROWS, PITCH), PAD_BYTE, np.uint8)
    s[:HF, :WF] = y
    s[CHROMA_ROW:CHROMA_ROW + (HF + 1) // 2, :2 * ((WF + 1) // 2)] = uv.reshape(uv.shape[0], -1)
    return s


def surface_to_frame(surface):
    return nv12_to_bgr_np(surface, HF, WF, chroma_row=CHROMA_ROW)


def through_nv12(colours):
    """What flat patches of these BGR colours become through bgr_to_nv12_np and nv12_to_bgr_np: [n,3] uint8."""
    patch = np.broadcast_to(np.asarray(colours, np.uint8)[:, None, None, :], (len(colours), 4, 4, 3))
    y, uv = bgr_to_nv12_np(patch)
    from tests.test_yuv_cpu import yuv_to_bgr_np
    return yuv_to_bgr_np(y, uv)[:, 0, 0, :]


def conversion_gain():
    """coco_h36m_np is linear in x and in y, each on its own: its matrices, read off the restatement on unit vectors -> (Jx, Jy [17,17], gain [17,2] = the row
    sums of |J|: how far an H36M coordinate can move when every COCO coordinate moves by at most 1)."""
    eye = np.zeros((17, 17, 3), F32)
    eye[np.arange(17), np.arange(17), :2] = 1.0
    out = coco_h36m_np(eye).astype(F64)        # [in, out, 3]
    Jx, Jy = out[..., 0].T, out[..., 1].T
    return Jx, Jy, np.stack((np.abs(Jx).sum(axis=1), np.abs(Jy).sum(axis=1)), axis=-1)


class Scene:
    """The planted truth and the painted frames of one stream.  ``shift``: moves every player (a second, different scene for the two-stream test)."""

    def __init__(self, seed=0, shift=(0.0, 0.0)):
        self.markers, self.torsos = palette()
        self.markers_seen, self.torsos_seen = through_nv12(self.markers), through_nv12(self.torsos)
        t = np.arange(TICKS, dtype=F64)
        moved = np.array([1.0, 1.0, 0.0])[:, None] * np.asarray(shift, F64)[None, :]                              # the edge player is never shifted
        centre = (START + moved)[None] + t[:, None, None] * VELOCITY[None]
        self.centre = centre                                                     # [T,3,2]
        self.boxes = np.concatenate((centre - (BOX_W / 2, BOX_H / 2), centre + (BOX_W / 2, BOX_H / 2)), axis=-1)       # [T,3,4] x1, y1, x2, y2
        j = np.arange(17, dtype=F64)
        wiggle = 0.8 * np.stack((np.sin(0.7 * t[:, None] + j[None]), np.cos(0.7 * t[:, None] + 2 * j[None])), axis=-1)  # [T,17,2]
        self.coco = centre[:, :, None, :] + (LAYOUTS - (0.0, BOX_H / 2))[None] + wiggle[:, None] * (1 + 0.1 * np.arange(3))[None, :, None, None]
        self.present = np.ones((TICKS, 3), bool)
        for p, (a, b) in ABSENT.items():
            self.present[a:b + 1, p] = False
        pix = np.rint(self.coco).astype(np.int64)
        self.pix = pix
        self.marked = self.present[:, :, None] & (pix[..., 0] >= 0) & (pix[..., 0] < WF) & (pix[..., 1] >= 0) & (pix[..., 1] < HF)     # [T,3,17]
        Jx, Jy, self.gain = conversion_gain()
        self.h36m = coco_h36m_np(np.concatenate((self.coco, np.ones(self.coco.shape[:-1] + (1,))), axis=-1).astype(F32))[..., :2].astype(F64)
        uses = (Jx != 0) | (Jy != 0)                                             # [out, in]
        self.h36m_marked = (self.marked[:, :, None, :] | ~uses[None, None]).all(axis=-1)           # an H36M joint needs every COCO joint it is made of
        self.frames = np.stack([self._paint(k, seed) for k in range(TICKS)])
        self.surfaces = np.stack([make_surface(f) for f in self.frames])

    def _paint(self, tick, seed):
        g = np.random.default_rng(1000 * seed + tick)
        frame = np.repeat((128 + g.integers(-12, 13, size=(HF, WF, 1))).astype(np.uint8), 3, axis=2)
        yy, xx = np.mgrid[0:HF, 0:WF]
        for p in range(3):
            if not self.present[tick, p]:
                continue
            cx, top = int(np.rint(self.centre[tick, p, 0])), int(np.rint(self.centre[tick, p, 1] - BOX_H / 2))
            x0, y0, x1, y1 = max(cx + TORSO[0], 0), max(top + TORSO[1], 0), min(cx + TORSO[2], WF - 1), min(top + TORSO[3], HF - 1)
            frame[y0:y1 + 1, x0:x1 + 1] = self.torsos[p]
        for p in range(3):
            for j in range(17):
                if self.marked[tick, p, j]:
                    x, y = self.pix[tick, p, j]
                    frame[(xx - x) ** 2 + (yy - y) ** 2 <= MARKER_R * MARKER_R] = self.markers[j]
        return frame


class StandIns:
    """The two stand-in networks of one scene on ``device``; every constant they need lies on the device before the first tick."""

    def __init__(self, scene, device="cpu"):
        dev = torch.device(device)
        new_w, new_h, pad_x, pad_y = plan_np(WF, HF, INP, INP)
        sx, sy = new_w / WF, new_h / HF
        base = np.zeros((TICKS, N_ROWS, 85), F32)
        cx = np.zeros((TICKS, 3), np.int64)
        cy = np.zeros((TICKS, 3), np.int64)
        for t in range(TICKS):
            for p in range(3):
                x1, y1, x2, y2 = scene.boxes[t, p]
                box = ((x1 + x2) / 2 * sx + pad_x, (y1 + y2) / 2 * sy + pad_y, (x2 - x1) * sx, (y2 - y1) * sy)
                cx[t, p] = int(np.clip(np.rint(((x1 + x2) / 2 + 0.5) * sx - 0.5 + pad_x), 0, INP - 1))
                cy[t, p] = int(np.clip(np.rint(((y1 + y2) / 2 + 0.5) * sy - 0.5 + pad_y), 0, INP - 1))
                if scene.present[t, p]:
                    base[t, PLAYER_ROWS[p], :5] = box + (0.9 - 0.05 * p,)
                    base[t, PLAYER_ROWS[p], 6] = 0.5
                    if p == 0:
                        base[t, DUPLICATE_ROW, :5] = (box[0] + 2.0, box[1] + 2.0, box[2], box[3], 0.55)
                        base[t, DUPLICATE_ROW, 6] = 0.5
            base[t, LOW_ROW, :7] = (300.0, 120.0, 40.0, 60.0, 0.2, 0.95, 0.1)
            base[t, OTHER_ROW, :7] = (100.0, 300.0, 40.0, 60.0, 0.9, 0.1, 0.99)
        self.base = torch.from_numpy(base).to(dev)
        self.cx, self.cy = torch.from_numpy(cx).to(dev), torch.from_numpy(cy).to(dev)
        self.torso_rgb = torch.from_numpy(scene.torsos_seen[:, ::-1].astype(F32).copy()).to(dev)                 # [3,3] R, G, B
        self.marker_rgb = torch.from_numpy(scene.markers_seen[:, ::-1].astype(F32).copy()).to(dev)               # [17,3]
        self.mean_rgb = torch.tensor(MEAN[::-1], dtype=torch.float32, device=dev).view(1, 3, 1, 1)               # plane k: frame channel 2 - k
        self.std_rgb = torch.tensor(STD[::-1], dtype=torch.float32, device=dev).view(1, 3, 1, 1)

    def detector(self, inputs, tick):
        """lb.inputs [1,3,INP,INP] (R, G, B planes, 0..1) -> prediction [1,N_ROWS,85] in letterbox coordinates."""
        pix = inputs[0][:, self.cy[tick], self.cx[tick]].t() * 255.0                                           # [3 players, 3 planes]
        match = ((pix - self.torso_rgb).abs().amax(dim=1) <= DET_TOL).to(torch.float32) * 0.95
        pred = self.base[tick:tick + 1].clone()
        live = (pred[0, 1:8:3, 4] > 0).to(torch.float32)
        pred[0, 1:8:3, 5] = match * live
        pred[0, DUPLICATE_ROW, 5] = match[0]
        return pred

    def pose_network(self, inputs):
        """r.inputs [P,3,h,w] -> heatmaps [P,17,h/4,w/4] in [0, 1]."""
        rgb = (inputs.to(torch.float32) * self.std_rgb + self.mean_rgb) * 255.0
        d = (rgb[:, None] - self.marker_rgb[None, :, :, None, None]).abs().amax(dim=2)
        return torch.nn.functional.avg_pool2d((1.0 - d / TAU).clamp(0.0, 1.0), 7, 4, 3)


# ---- the composed restatement ----------------------------------------------------------------------------------------------------------------------------
def op_frame(surface):
    return surface_to_frame(surface)


def op_letterbox(frame):
    return letterbox_np(frame, INP)


def op_detect(pred):
    return detect_decode_np(pred, WF, HF, INP, confidence=CONFIDENCE)


def op_track(trk, boxes, count):
    return sort_update_np(trk, np.ascontiguousarray(boxes, F32), count)


def op_crop(frame, persons):
    return crop_persons_np(frame, persons, size=SIZE)


def op_decode(hm, center, scale):
    return coco_h36m_np(heatmap_decode_np(hm, center, scale))


def op_filter(state, kp, arrays, tick):
    return smooth_ref.tracked_np(state, FILTER, kp, arrays, "persons", NUM_PERSON, tick, True)


def op_draw(frame, kp, valid):
    return draw_poses_np(frame[None], kp[None], valid[None], colors=wheel(16), min_score=MIN_SCORE, boxed=True)[0]


def op_surface(painted):
    return bgr_to_nv12_np(painted)


OPS = dict(frame=op_frame, letterbox=op_letterbox, detect=op_detect, track=op_track, crop=op_crop, decode=op_decode, filter=op_filter, draw=op_draw,
           surface=op_surface)


def track_arrays(r, slots=SLOTS):
    """One stream's sort_update_np result -> the padded [1,slots] arrays a TrackResult holds (ids -1, slot 0, born 0 past count)."""
    n = r["count"]
    ids, slot, born = np.full((1, slots), -1, np.int32), np.zeros((1, slots), np.int32), np.zeros((1, slots), np.int32)
    ids[0, :n], slot[0, :n], born[0, :n] = r["ids"], r["slot"], r["born"]
    return dict(ids=ids, slot=slot, born=born, count=np.array([n], np.int32))


def padded_persons(r, num_person=NUM_PERSON):
    p = np.zeros((num_person, 4), F32)
    p[:r["person_count"]] = r["persons"].astype(F32)
    return p


def new_state(min_hits=0):
    return dict(trk=new_tracker(slots=SLOTS, max_age=MAX_AGE, min_hits=min_hits, num_person=NUM_PERSON), f2=smooth_ref.new_state(SLOTS, 17, 2), tick=0)


def tick_np(state, surface, nets, ops=OPS):
    """One tick of the whole chain through the restatements, the stand-ins on the CPU between them -> every stage's output."""
    o = SimpleNamespace()
    o.frame = ops["frame"](surface)
    o.lb = ops["letterbox"](o.frame)
    o.pred = nets.detector(torch.from_numpy(o.lb), state["tick"]).numpy()
    o.boxes, o.count, o.candidates, o.index = ops["detect"](o.pred)
    o.track = ops["track"](state["trk"], o.boxes[0], o.count[0])
    o.persons = padded_persons(o.track)
    o.inputs, o.center, o.scale = ops["crop"](o.frame, o.persons)
    o.hm = nets.pose_network(torch.from_numpy(o.inputs)).numpy()
    o.kp_raw = ops["decode"](o.hm, o.center, o.scale)
    o.kp, row_slot, _, _ = ops["filter"](state["f2"], o.kp_raw, track_arrays(o.track), state["tick"])
    o.valid = row_slot >= 0
    o.painted = ops["draw"](o.frame, o.kp, o.valid)
    o.enc_y, o.enc_uv = ops["surface"](o.painted)
    state["tick"] += 1
    return o


def run_np(scene, min_hits=0, ops=OPS, ticks=TICKS):
    nets, state = StandIns(scene), new_state(min_hits)
    return [tick_np(state, scene.surfaces[t], nets, ops) for t in range(ticks)]


# ---- the plant against a tick's keypoints -----------------------------------------------------------------------------------------------------------------
def bound(scale):
    """BOUND per axis for the COCO joints of a crop made with ``scale`` [2]: 0.75 heatmap cell -- half a cell from the argmax, a quarter from the refinement
    -- in frame pixels, plus 1 px for the marker's rounding to a pixel and the chroma's 2 x 2 siting.  A cell is scale[0] * 200 / HM_W pixels on BOTH axes:
    only scale[0] enters the crop's and the decode's geometry (kasf.h; crop_geometry_np: ky = kx), and HM_H / HM_W is the crop's own aspect."""
    return 0.75 * float(scale[0]) * 200.0 / HM_W + 1.0


def owner_and_ratio(scene, tick, kp_row, scale_row):
    """The planted player whose joints lie nearest to keypoints [17,>=2] (H36M), and the worst |error| / (gain * BOUND) over that player's marked joints and
    both axes -> (player or None when nobody is present, ratio, worst error in px)."""
    best = (None, np.inf, np.inf)
    for p in range(3):
        if not scene.present[tick, p]:
            continue
        m = scene.h36m_marked[tick, p]
        err = np.abs(np.asarray(kp_row, F64)[m, :2] - scene.h36m[tick, p][m])
        ratio = float((err / (scene.gain[m] * bound(scale_row))).max())
        if ratio < best[1]:
            best = (p, ratio, float(err.max()))
    return best
