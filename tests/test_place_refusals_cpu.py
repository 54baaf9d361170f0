"""Every refusal of kasf_pose_place (csrc/api_place.hip): code 2, the message in kasf_last_error(), reached with null or bogus host pointers so that nothing is
launched and no GPU is needed (tests/refusal_cases.py's caller, table form and generated null / all_wrong / pair cases; the table is this file's own).  Every
message literal of api_place.hip is hit by some case.  Then the refusals of ``place_poses``, all raised before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import refusal_cases as R

API = os.path.join(R.ROOT, "kasportsformer_amd", "csrc", "api_place.hip")
NAN, INF = float("nan"), float("inf")


class Place(C.Structure):        # kasf_place_params
    _fields_ = [("min_score", C.c_float), ("weighted", C.c_int32), ("iterations", C.c_int32), ("delta", C.c_float), ("min_joints", C.c_int32)]


def place(**kw):
    return Place(**{**dict(min_score=0.3, weighted=1, iterations=4, delta=3.0, min_joints=4), **kw})


_DELTA = "pose_place: delta must be finite and > 0"
# (case, overrides, message) in the order of the entry's checks
CASES = [
    ("frames", dict(frames=-1), "pose_place: frames must be >= 0"),
    ("score_nan", dict(params=place(min_score=NAN)), "pose_place: min_score must be finite"),
    ("score_inf", dict(params=place(min_score=INF)), "pose_place: min_score must be finite"),
    ("weighted", dict(params=place(weighted=2)), "pose_place: weighted must be 0 or 1"),
    ("weighted_neg", dict(params=place(weighted=-1)), "pose_place: weighted must be 0 or 1"),
    ("iterations_neg", dict(params=place(iterations=-1)), "pose_place: iterations must be in [0, 8]"),
    ("iterations_big", dict(params=place(iterations=9)), "pose_place: iterations must be in [0, 8]"),
    ("delta_zero", dict(params=place(delta=0.0)), _DELTA), ("delta_neg", dict(params=place(delta=-1.0)), _DELTA),
    ("delta_nan", dict(params=place(delta=NAN)), _DELTA), ("delta_inf", dict(params=place(delta=INF)), _DELTA),
    ("joints_small", dict(params=place(min_joints=1)), "pose_place: min_joints must be in [2, 17]"),
    ("joints_big", dict(params=place(min_joints=18)), "pose_place: min_joints must be in [2, 17]"),
    ("out_is_poses", dict(out=R.SAME("poses")), "pose_place: out must be an array of its own, neither poses nor keypoints"),
    ("out_is_keypoints", dict(out=R.SAME("keypoints")), "pose_place: out must be an array of its own, neither poses nor keypoints"),
]
OPTIONAL = ("lengths", "root", "residual", "scale", "state")
ENTRY = ("kasf_pose_place", dict(frames=4, params=place()), [(c, o) for c, o, _ in CASES], OPTIONAL)


def library():
    lib = C.CDLL(R.LIB_PATH)
    lib.kasf_last_error.restype = C.c_char_p
    return lib


def replay():
    lib, said = library(), {}
    for cid, overrides, first in R.cases_of(ENTRY):
        code = R._call(lib, ENTRY[0], ENTRY[1], overrides)
        said[cid] = lib.kasf_last_error().decode()
        assert code == 2, f"{cid}: code {code} ({said[cid]}): the call was not refused with 2"
        assert first is None or said[cid] == said[first], f"{cid}: says {said[cid]!r}, not {said[first]!r}"
    return said


def test_every_refusal_is_code_2_with_its_message():
    said = replay()
    for cid, _, message in CASES:
        assert said[cid] == message, cid
    nulls = {cid for cid in said if cid.startswith("null:")}
    assert nulls == {"null:poses", "null:keypoints", "null:camera", "null:params", "null:out"}          # the five optional ones may be NULL
    assert all(said[cid] == "null pointer argument" for cid in nulls)
    assert said["all_wrong"] == "pose_place: frames must be >= 0"
    # frames == 0 succeeds without a launch, before it looks at a data pointer; the parameters are checked all the same
    lib = library()
    nothing = {p: None for p in ("poses", "keypoints", "camera", "out") + OPTIONAL}
    assert R._call(lib, ENTRY[0], {**ENTRY[1], "frames": 0}, nothing) == 0
    assert R._call(lib, ENTRY[0], {**ENTRY[1], "frames": 0, "params": place(iterations=9)}, nothing) == 2
    assert R._call(lib, ENTRY[0], {**ENTRY[1], "frames": 0, "params": place(iterations=0, min_joints=17, weighted=0)}, nothing) == 0


def test_every_message_of_the_file_has_a_case():
    text = re.sub(r"//[^\n]*", "", open(API).read())
    assert set(re.findall(r"^(?:int|int64_t) (kasf_\w+)\(", text, flags=re.M)) == {ENTRY[0]}
    said = set(replay().values())
    literals = [s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', text) if len(s) >= 8 and not s.endswith(".h")]
    assert len(literals) >= 7
    missing = [s for s in literals if not any(s in m for m in said)]
    assert not missing, missing


def test_the_symbol_is_declared_in_the_header_and_exported():
    assert ENTRY[0] in R.PROTOS and [p for p, _, _ in R.PROTOS[ENTRY[0]][1]] == [
        "poses", "keypoints", "frames", "camera", "camera_per_frame", "lengths", "lengths_per_frame", "params", "out", "root", "residual", "scale", "state", "stream"]
    lib = library()
    assert hasattr(lib, ENTRY[0])
    lib.kasf_version.restype = C.c_int
    assert lib.kasf_version() == 12                                      # additive: the ABI version stays


def test_the_ctypes_struct_matches_the_header():
    from kasportsformer_amd import _lib
    assert C.sizeof(_lib.KasfPlaceParams) == C.sizeof(Place) == 20
    assert [(n, C.sizeof(t)) for n, t in _lib.KasfPlaceParams._fields_] == [(n, C.sizeof(t)) for n, t in Place._fields_]
    header = open(os.path.join(R.ROOT, "include", "kasf.h")).read()
    body = re.search(r"typedef struct kasf_place_params \{(.*?)\} kasf_place_params;", header, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [n for n, _ in Place._fields_]
    assert len(_lib.SIGNATURES["kasf_pose_place"][1]) == len(R.PROTOS[ENTRY[0]][1]) == 14


POSES, KP, CAM = np.zeros((5, 17, 3), np.float32), np.zeros((5, 17, 3), np.float32), np.array([1500, 1500, 960, 540], np.float32)


@pytest.mark.parametrize("kw,error,text", [
    (dict(min_score="0.3"), TypeError, "place_poses: min_score must be a number"),
    (dict(min_score=NAN), ValueError, "place_poses: min_score must be finite"),
    (dict(delta=True), TypeError, "place_poses: delta must be a number"),
    (dict(delta=INF), ValueError, "place_poses: delta must be finite"),
    (dict(delta=0.0), ValueError, "place_poses: delta must be > 0 pixels"),
    (dict(delta=-2.0), ValueError, "place_poses: delta must be > 0 pixels"),
    (dict(weighted=1), TypeError, "place_poses: weighted must be a bool"),
    (dict(iterations=-1), ValueError, "place_poses: iterations must be in [0, 8]"),
    (dict(iterations=9), ValueError, "place_poses: iterations must be in [0, 8]"),
    (dict(iterations=2.0), TypeError, "place_poses: iterations must be an int"),
    (dict(min_joints=1), ValueError, "place_poses: min_joints must be in [2, 17]"),
    (dict(min_joints=18), ValueError, "place_poses: min_joints must be in [2, 17]"),
    (dict(min_joints=True), TypeError, "place_poses: min_joints must be an int"),
    (dict(poses=[[0.0]]), TypeError, "place_poses: poses must be a numpy array or a torch tensor"),
    (dict(poses=POSES.astype(np.float64)), TypeError, "place_poses: poses must be float32"),
    (dict(keypoints=KP.astype(np.float16)), TypeError, "place_poses: keypoints must be float32"),
    (dict(poses=np.zeros((5, 17, 2), np.float32)), ValueError, "place_poses: expected poses of [...,17,3]"),
    (dict(poses=np.zeros(3, np.float32)), ValueError, "place_poses: expected poses of [...,17,3]"),
    (dict(keypoints=np.zeros((4, 17, 3), np.float32)), ValueError, "place_poses: keypoints must have the poses' shape"),
    (dict(keypoints=np.zeros((5, 17, 2), np.float32)), ValueError, "place_poses: keypoints must have the poses' shape"),
    (dict(camera=np.zeros(3, np.float32)), ValueError, "place_poses: camera must be [4] (fx, fy, cx, cy) or [5, 4]"),
    (dict(camera=np.zeros((4, 4), np.float32)), ValueError, "place_poses: camera must be [4] (fx, fy, cx, cy) or [5, 4]"),
    (dict(camera=[1500.0, 1500.0, 960.0, 540.0]), TypeError, "place_poses: camera must be a numpy array or a torch tensor"),
    (dict(camera=CAM.astype(np.float64)), TypeError, "place_poses: camera must be float32"),
    (dict(metric_lengths=np.zeros(17, np.float32)), ValueError, "place_poses: metric_lengths must be [16] (metres per bone) or [5, 16]"),
    (dict(metric_lengths=np.zeros((5, 17), np.float32)), ValueError, "place_poses: metric_lengths must be [16] (metres per bone) or [5, 16]"),
    (dict(metric_lengths=np.zeros(16, np.float64)), TypeError, "place_poses: metric_lengths must be float32"),
    (dict(device="cpu"), RuntimeError, "place_poses: device must be a GPU"),
])
def test_place_poses_refuses_before_any_launch(kw, error, text):
    from kasportsformer_amd import place_poses
    kw = dict(kw)
    with pytest.raises(error) as e:
        place_poses(kw.pop("poses", POSES), kw.pop("keypoints", KP), kw.pop("camera", CAM), **kw)
    assert str(e.value).startswith(text), str(e.value)


def test_the_parameters_as_the_entry_takes_them():
    from kasportsformer_amd.place import place_params
    p = place_params()
    assert (p.weighted, p.iterations, p.min_joints) == (1, 4, 4) and p.min_score == np.float32(0.3) and p.delta == 3.0
    p = place_params(0, False, np.int64(8), 1, 17)
    assert (p.min_score, p.weighted, p.iterations, p.delta, p.min_joints) == (0.0, 0, 8, 1.0, 17)


def test_the_bone_table_file(tmp_path):
    from kasportsformer_amd.place import load_bone_table
    good = np.linspace(0.1, 0.5, 16)
    np.save(tmp_path / "t.npy", good)
    assert load_bone_table(str(tmp_path / "t.npy")).dtype == np.float32
    for name, bad in (("shape", np.ones(17)), ("nan", np.r_[np.nan, np.ones(15)]), ("negative", np.r_[-1.0, np.ones(15)]), ("zeros", np.zeros(16)),
                      ("text", np.array(["a"] * 16))):
        np.save(tmp_path / f"{name}.npy", bad)
        with pytest.raises(ValueError):
            load_bone_table(str(tmp_path / f"{name}.npy"))
