"""csrc/k_track.hip without a GPU: the kernel's own source compiled for the host with g++ behind a lockstep emulation of the wavefront (tests/host_emul/:
64 threads, a barrier at every shuffle, ballot and __syncthreads) and held to ``sort_update_np`` with the checks of tests/test_gpu_track.py -- every discrete
output and counter exact, x, P and boxes to 1e-12.  It shows the kernel's logic and its fp64 operation order; what only the device can show (its divide and
square root, the real shuffles, LDS) stays with tests/test_gpu_track.py.  The first ticks of each case, to stay quick: 64 threads meet at ~10,000 barriers a tick.
"""
import ctypes as C

import numpy as np
import pytest

from tests.host_emul import build, vp
from tests.test_gpu_track import check_tick
from tests.test_track_cpu import CASES, pad, run_np

TICKS = {"greedy": 3, "overflow": 16, "max_age2": 14, "birth_death": 13, "bad_rows": 8, "hold_on": 10, "hold_off": 10, "demo": 12, "default": 20, "full64": 3}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "track_host", "emul_track.cpp")
    lib.emul_state_bytes.restype = C.c_int64
    return lib


class HostTracker:
    """One stream of the emulated kernel, with the state unpacked as ``SortTracker.state()`` does."""

    def __init__(self, lib, slots=32, max_age=1, min_hits=3, iou_threshold=0.3, num_person=1, hold_last=False):
        self.lib, self.S, self.p = lib, slots, (max_age, min_hits, iou_threshold, num_person, int(hold_last))
        self.state = np.zeros(lib.emul_state_bytes(slots, 64), np.uint8)

    def update(self, dets, count):
        S, (max_age, min_hits, thr, NP, hold) = self.S, self.p
        dets, cnt = np.ascontiguousarray(dets, np.float32), np.array([count], np.int32)
        o = dict(boxes=np.full((S, 4), 5, np.float32), ids=np.full(S, 5, np.int32), slot=np.full(S, 5, np.int32), born=np.full(S, 5, np.int32),
                 count=np.full(1, 5, np.int32), dropped=np.full(1, 5, np.int32), persons=np.full((NP, 4), 5, np.float32), person_count=np.full(1, 5, np.int32))
        self.lib.emul_update(vp(self.state), 1, S, 64, vp(dets), dets.shape[0], C.c_int64(0), C.c_int64(dets.shape[1]), vp(cnt), max_age, min_hits, C.c_float(thr),
                             NP, hold, vp(o["boxes"]), vp(o["ids"]), vp(o["slot"]), vp(o["born"]), vp(o["count"]), vp(o["dropped"]), vp(o["persons"]),
                             vp(o["person_count"]))
        for k in ("count", "dropped", "person_count"):
            o[k] = o[k][0]
        o["state"] = self.unpack()
        return o

    def unpack(self):
        S, st = self.S, self.state
        hdr, o = st[:64].view(np.int32), 64
        x = st[o:o + 56 * S].view(np.float64).reshape(7, S).T.copy()
        blk = st[o + 56 * S:o + 160 * S].view(np.float64).reshape(13, S)
        ints = st[o + 160 * S:o + 184 * S].view(np.int32).reshape(6, S)
        P = np.zeros((S, 7, 7))
        for k in range(3):
            P[:, k, k], P[:, k, k + 4], P[:, k + 4, k], P[:, k + 4, k + 4] = blk[4 * k], blk[4 * k + 1], blk[4 * k + 2], blk[4 * k + 3]
        P[:, 3, 3] = blk[12]
        with np.errstate(all="ignore"):
            w = np.sqrt(x[:, 2] * x[:, 3])
            h = x[:, 2] / w
            boxes = np.stack((x[:, 0] - w / 2, x[:, 1] - h / 2, x[:, 0] + w / 2, x[:, 1] + h / 2), -1)
        boxes[hdr[0]:] = 0
        return dict(x=x, P=P, boxes=boxes, ids=ints[0].copy(), slot=ints[1].copy(), time_since_update=ints[2].copy(), hits=ints[3].copy(),
                    hit_streak=ints[4].copy(), age=ints[5].copy(), tracks=hdr[0], next_id=hdr[1], ticks=hdr[2])


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_source_on_the_host_follows_the_restatement(name, emul):
    params, seq, rows = CASES[name]
    ticks = TICKS[name]
    dets, count = pad(seq, rows)
    want = run_np(params, seq[:ticks], states=True)
    trk = HostTracker(emul, **params)
    for t in range(ticks):
        check_tick(trk.update(dets[t], count[t]), want[t], (name, t))
