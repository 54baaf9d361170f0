#!/usr/bin/env python3
"""Generate the fixture of the SORT tracker from the REAL reference class (run in the build container only).

    python tests/golden/make_track_golden.py       # needs the reference checkout (make_lift_golden.REF)

Imports ``demo/lib/sort/sort.py`` and calls its ``Sort(max_age, min_hits).update(dets)`` as it is, tick by tick, on the sequences of
tests/test_track_cpu.py (``CASES``, the ones in ``FIXTURE_CASES``: what the reference can run).  Three modules it imports are not installed here and are
shimmed IN THIS PROCESS ONLY:

  numba     ``jit`` is the identity: ``iou`` runs as the numpy code it is.
  skimage   imported for its ``io``, which ``Sort`` does not use: an empty module.
  filterpy  ``KalmanFilter``: a small class WRITTEN HERE with the predict and update of filterpy's published form (x = F x, P = F P F^T + Q; y = z - H x,
            S = H P H^T + R, K = P H^T S^-1, x = x + K y, P = (I - K H) P (I - K H)^T + K R K^T).  THE FILTER ARITHMETIC IS THIS PROJECT'S RESTATEMENT, not
            filterpy's code: the fixture pins the reference's bookkeeping -- association, threshold, births, deaths, output order, ids -- and the boxes that
            bookkeeping produces through this filter.

``KalmanBoxTracker.count`` is a class attribute shared by every ``Sort``; it is set back to 0 in front of each sequence, which is what a fresh process would
see.  Writes tensors only:

  track_sort.npz, per case c
    c_dets [T, rows, 5] float32, c_count [T] int32     the detections as tests/test_track_cpu.py pads them; the reference is given dets[t, :count[t]] as float64
    c_ret [T, K, 5] float64, c_ret_count [T] int32     what Sort.update returned on tick t (x1, y1, x2, y2, id + 1; newest track first), zero-padded to K rows
    c_params [2] int32                                 max_age, min_hits
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from make_lift_golden import REF  # noqa: E402


class KalmanFilter:
    def __init__(self, dim_x, dim_z):
        self.x, self.P, self.Q = np.zeros((dim_x, 1)), np.eye(dim_x), np.eye(dim_x)
        self.F, self.H, self.R = np.eye(dim_x), np.zeros((dim_z, dim_x)), np.eye(dim_z)
        self._I = np.eye(dim_x)

    def predict(self):
        self.x = np.dot(self.F, self.x)
        self.P = np.dot(np.dot(self.F, self.P), self.F.T) + self.Q

    def update(self, z):
        z = np.asarray(z, np.float64).reshape(-1, 1)
        y = z - np.dot(self.H, self.x)
        PHT = np.dot(self.P, self.H.T)
        S = np.dot(self.H, PHT) + self.R
        K = np.dot(PHT, np.linalg.inv(S))
        self.x = self.x + np.dot(K, y)
        I_KH = self._I - np.dot(K, self.H)
        self.P = np.dot(np.dot(I_KH, self.P), I_KH.T) + np.dot(np.dot(K, self.R), K.T)


def shim_missing_modules():
    for name in ("numba", "skimage", "skimage.io", "filterpy", "filterpy.kalman"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
            print("shimmed", name)
    if not hasattr(sys.modules["numba"], "jit"):
        sys.modules["numba"].jit = lambda f: f
    if "io" not in vars(sys.modules["skimage"]):
        sys.modules["skimage"].io = sys.modules["skimage.io"]
    if not hasattr(sys.modules["filterpy.kalman"], "KalmanFilter"):
        sys.modules["filterpy"].kalman = sys.modules["filterpy.kalman"]
        sys.modules["filterpy.kalman"].KalmanFilter = KalmanFilter


def main():
    shim_missing_modules()
    sys.path.insert(0, os.path.join(REF, "demo"))
    from lib.sort import sort as ref
    from tests.test_track_cpu import CASES, FIXTURE_CASES, pad

    out = {}
    for name in FIXTURE_CASES:
        params, seq, rows = CASES[name]
        assert not params.get("hold_last") and set(params) <= {"slots", "max_age", "min_hits", "num_person"}
        dets, count = pad(seq, rows)
        ref.KalmanBoxTracker.count = 0
        tracker = ref.Sort(max_age=params.get("max_age", 1), min_hits=params.get("min_hits", 3))
        rets = [np.asarray(tracker.update(dets[t, :count[t]].astype(np.float64)), np.float64).reshape(-1, 5) for t in range(len(seq))]
        K = max(1, max(len(r) for r in rets))
        assert K <= params["slots"], "the reference held more tracks than the case has slots"
        ret = np.zeros((len(seq), K, 5))
        for t, r in enumerate(rets):
            ret[t, :len(r)] = r
        out.update({f"{name}_dets": dets, f"{name}_count": count, f"{name}_ret": ret, f"{name}_ret_count": np.array([len(r) for r in rets], np.int32),
                    f"{name}_params": np.array([params.get("max_age", 1), params.get("min_hits", 3)], np.int32)})
    path = os.path.join(HERE, "track_sort.npz")
    np.savez_compressed(path, **out)
    print("wrote track_sort.npz:", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
