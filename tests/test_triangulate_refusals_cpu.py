"""Every refusal of kasf_keypoints_triangulate and kasf_keypoints_undistort (csrc/api_triangulate.hip): code 2, the message in kasf_last_error(), reached with
null or bogus host pointers so that nothing is launched and no GPU is needed (tests/refusal_cases.py's caller, table form and generated null / all_wrong / pair
cases; the tables are this file's own).  Every message literal of api_triangulate.hip is hit by some case.  Then the refusals of ``triangulate_keypoints``,
``undistort_keypoints`` and ``camera_row``, all raised before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import refusal_cases as R

API = os.path.join(R.ROOT, "kasportsformer_amd", "csrc", "api_triangulate.hip")
NAN, INF = float("nan"), float("inf")


class Tri(C.Structure):          # kasf_triangulate_params
    _fields_ = [("min_score", C.c_float), ("weighted", C.c_int32), ("iterations", C.c_int32), ("delta", C.c_float), ("min_views", C.c_int32),
                ("undistort_iterations", C.c_int32)]


def tri(**kw):
    return Tri(**{**dict(min_score=0.3, weighted=1, iterations=4, delta=3.0, min_views=2, undistort_iterations=5), **kw})


T, U = "keypoints_triangulate: ", "keypoints_undistort: "
# (case, overrides, message) in the order of the entry's checks
TRI_CASES = [
    ("views_small", dict(views=1), T + "views must be in [2, 16]"), ("views_big", dict(views=17), T + "views must be in [2, 16]"),
    ("M", dict(M=-17), T + "M must be >= 0"),
    ("ppf", dict(points_per_frame=0), T + "points_per_frame must be >= 1"),
    ("multiple", dict(M=35, points_per_frame=17), T + "M must be a multiple of points_per_frame"),
    ("score_nan", dict(params=tri(min_score=NAN)), T + "min_score must be finite"), ("score_inf", dict(params=tri(min_score=-INF)), T + "min_score must be finite"),
    ("weighted", dict(params=tri(weighted=2)), T + "weighted must be 0 or 1"), ("weighted_neg", dict(params=tri(weighted=-1)), T + "weighted must be 0 or 1"),
    ("iterations_neg", dict(params=tri(iterations=-1)), T + "iterations must be in [0, 8]"),
    ("iterations_big", dict(params=tri(iterations=9)), T + "iterations must be in [0, 8]"),
    ("delta_zero", dict(params=tri(delta=0.0)), T + "delta must be finite and > 0"), ("delta_neg", dict(params=tri(delta=-1.0)), T + "delta must be finite and > 0"),
    ("delta_nan", dict(params=tri(delta=NAN)), T + "delta must be finite and > 0"), ("delta_inf", dict(params=tri(delta=INF)), T + "delta must be finite and > 0"),
    ("views_min_small", dict(params=tri(min_views=1)), T + "min_views must be in [2, 16]"),
    ("views_min_big", dict(params=tri(min_views=17)), T + "min_views must be in [2, 16]"),
    ("rounds_neg", dict(params=tri(undistort_iterations=-1)), T + "undistort_iterations must be in [0, 20]"),
    ("rounds_big", dict(params=tri(undistort_iterations=21)), T + "undistort_iterations must be in [0, 20]"),
    ("points_is_keypoints", dict(points=R.SAME("keypoints")), T + "points must be an array of its own, not keypoints"),
]
UND_CASES = [
    ("M", dict(M=-1), U + "M must be >= 0"),
    ("ppf", dict(points_per_frame=0), U + "points_per_frame must be >= 1"),
    ("multiple", dict(M=18, points_per_frame=17), U + "M must be a multiple of points_per_frame"),
    ("rounds_neg", dict(iterations=-1), U + "iterations must be in [0, 20]"), ("rounds_big", dict(iterations=21), U + "iterations must be in [0, 20]"),
    ("out_is_keypoints", dict(out=R.SAME("keypoints")), U + "out must be an array of its own, not keypoints"),
]
TRI_OPTIONAL = ("residual", "used", "state", "view_residual")
ENTRIES = {
    "kasf_keypoints_triangulate": (dict(views=3, M=34, points_per_frame=17, params=tri()), TRI_CASES, TRI_OPTIONAL),
    "kasf_keypoints_undistort": (dict(M=34, points_per_frame=17, iterations=5), UND_CASES, ()),
}


def entry(name):
    base, cases, optional = ENTRIES[name]
    return (name, base, [(c, o) for c, o, _ in cases], optional)


def library():
    lib = C.CDLL(R.LIB_PATH)
    lib.kasf_last_error.restype = C.c_char_p
    return lib


def replay(name):
    lib, said, e = library(), {}, entry(name)
    for cid, overrides, first in R.cases_of(e):
        code = R._call(lib, e[0], e[1], overrides)
        said[cid] = lib.kasf_last_error().decode()
        assert code == 2, f"{name} {cid}: code {code} ({said[cid]}): the call was not refused with 2"
        assert first is None or said[cid] == said[first], f"{name} {cid}: says {said[cid]!r}, not {said[first]!r}"
    return said


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_refusal_is_code_2_with_its_message(name):
    said = replay(name)
    for cid, _, message in ENTRIES[name][1]:
        assert said[cid] == message, cid
    nulls = {cid for cid in said if cid.startswith("null:")}
    want = {"null:keypoints", "null:cameras", "null:params", "null:points"} if name.endswith("triangulate") else {"null:keypoints", "null:camera", "null:out"}
    assert nulls == want                                                 # the four optional outputs may be NULL
    assert all(said[cid] == "null pointer argument" for cid in nulls)
    assert said["all_wrong"] == ENTRIES[name][1][0][2]


def test_nothing_to_do_succeeds_without_a_launch():
    """M == 0 returns 0 before it looks at a data pointer; the parameters are checked all the same."""
    lib = library()
    name, base = "kasf_keypoints_triangulate", ENTRIES["kasf_keypoints_triangulate"][0]
    nothing = {p: None for p in ("keypoints", "cameras", "points") + TRI_OPTIONAL}
    assert R._call(lib, name, {**base, "M": 0}, nothing) == 0
    assert R._call(lib, name, {**base, "M": 0, "params": tri(iterations=9)}, nothing) == 2
    assert R._call(lib, name, {**base, "M": 0, "views": 1}, nothing) == 2
    assert R._call(lib, name, {**base, "M": 0, "views": 16, "params": tri(iterations=0, min_views=16, weighted=0, undistort_iterations=20)}, nothing) == 0
    und = {p: None for p in ("keypoints", "camera", "out")}
    assert R._call(lib, "kasf_keypoints_undistort", {"M": 0, "points_per_frame": 1, "iterations": 0}, und) == 0
    assert R._call(lib, "kasf_keypoints_undistort", {"M": 0, "points_per_frame": 1, "iterations": 21}, und) == 2


def test_every_message_of_the_file_has_a_case():
    text = re.sub(r"//[^\n]*", "", open(API).read())
    assert set(re.findall(r"^(?:int|int64_t) (kasf_\w+)\(", text, flags=re.M)) == set(ENTRIES)
    said = set(replay("kasf_keypoints_triangulate").values()) | set(replay("kasf_keypoints_undistort").values())
    literals = [s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', text) if len(s) >= 8 and not s.endswith(".h")]
    assert len(literals) >= 18
    missing = [s for s in literals if not any(s in m for m in said)]
    assert not missing, missing


def test_the_symbols_are_declared_in_the_header_and_exported():
    assert [p for p, _, _ in R.PROTOS["kasf_keypoints_triangulate"][1]] == [
        "keypoints", "views", "M", "points_per_frame", "cameras", "cameras_per_frame", "params", "points", "residual", "used", "state", "view_residual", "stream"]
    assert [p for p, _, _ in R.PROTOS["kasf_keypoints_undistort"][1]] == [
        "keypoints", "M", "points_per_frame", "camera", "camera_per_frame", "iterations", "out", "stream"]
    lib = library()
    assert all(hasattr(lib, name) for name in ENTRIES)
    lib.kasf_version.restype = C.c_int
    assert lib.kasf_version() == 12                                      # additive: the ABI version stays


def test_the_ctypes_struct_matches_the_header():
    from kasportsformer_amd import _lib
    assert C.sizeof(_lib.KasfTriangulateParams) == C.sizeof(Tri) == 24
    assert [(n, C.sizeof(t)) for n, t in _lib.KasfTriangulateParams._fields_] == [(n, C.sizeof(t)) for n, t in Tri._fields_]
    header = open(os.path.join(R.ROOT, "include", "kasf.h")).read()
    body = re.search(r"typedef struct kasf_triangulate_params \{(.*?)\} kasf_triangulate_params;", header, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [n for n, _ in Tri._fields_]
    assert len(_lib.SIGNATURES["kasf_keypoints_triangulate"][1]) == len(R.PROTOS["kasf_keypoints_triangulate"][1]) == 13
    assert len(_lib.SIGNATURES["kasf_keypoints_undistort"][1]) == len(R.PROTOS["kasf_keypoints_undistort"][1]) == 8


KP = np.zeros((3, 5, 17, 3), np.float32)
CAMS = np.zeros((3, 21), np.float32)
W = "triangulate_keypoints: "


@pytest.mark.parametrize("kw,error,text", [
    (dict(min_score="0.3"), TypeError, W + "min_score must be a number"),
    (dict(min_score=NAN), ValueError, W + "min_score must be finite"),
    (dict(delta=True), TypeError, W + "delta must be a number"),
    (dict(delta=INF), ValueError, W + "delta must be finite"),
    (dict(delta=0.0), ValueError, W + "delta must be > 0 pixels"),
    (dict(weighted=1), TypeError, W + "weighted must be a bool"),
    (dict(iterations=-1), ValueError, W + "iterations must be in [0, 8]"),
    (dict(iterations=9), ValueError, W + "iterations must be in [0, 8]"),
    (dict(iterations=2.0), TypeError, W + "iterations must be an int"),
    (dict(min_views=1), ValueError, W + "min_views must be in [2, 16]"),
    (dict(min_views=17), ValueError, W + "min_views must be in [2, 16]"),
    (dict(min_views=True), TypeError, W + "min_views must be an int"),
    (dict(undistort_iterations=-1), ValueError, W + "undistort_iterations must be in [0, 20]"),
    (dict(undistort_iterations=21), ValueError, W + "undistort_iterations must be in [0, 20]"),
    (dict(undistort_iterations=5.0), TypeError, W + "undistort_iterations must be an int"),
    (dict(view_residual=1), TypeError, W + "view_residual must be a bool"),
    (dict(keypoints="kp"), TypeError, W + "keypoints must be a numpy array or a torch tensor"),
    (dict(keypoints=KP.astype(np.float64)), TypeError, W + "keypoints must be float32"),
    (dict(keypoints=[KP[0], KP[1].astype(np.float16), KP[2]]), TypeError, W + "keypoints[1] must be float32"),
    (dict(keypoints=[KP[0], KP[1, :4], KP[2]]), ValueError, W + "every camera's keypoints must have one shape"),
    (dict(keypoints=[KP[0]]), ValueError, W + "expected the keypoints of 2 to 16 cameras, got 1"),
    (dict(keypoints=np.zeros((17, 5, 17, 3), np.float32)), ValueError, W + "expected the keypoints of 2 to 16 cameras, got 17"),
    (dict(keypoints=np.zeros((3, 5, 17, 2), np.float32)), ValueError, W + "expected keypoints of [C,...,J,3]"),
    (dict(keypoints=np.zeros((3, 3), np.float32)), ValueError, W + "expected keypoints of [C,...,J,3]"),
    (dict(keypoints=np.zeros((3, 5, 0, 3), np.float32)), ValueError, W + "expected keypoints of [C,...,J,3]"),
    (dict(cameras=np.zeros((3, 20), np.float32)), ValueError, W + "cameras must be [3, 21] (fx, fy, cx, cy, k1, k2, p1, p2, k3, R, t) or [3, 5, 21]"),
    (dict(cameras=np.zeros((2, 21), np.float32)), ValueError, W + "cameras must be [3, 21]"),
    (dict(cameras=np.zeros((3, 4, 21), np.float32)), ValueError, W + "cameras must be [3, 21]"),
    (dict(cameras=CAMS.tolist()), TypeError, W + "cameras must be a numpy array or a torch tensor"),
    (dict(cameras=CAMS.astype(np.float64)), TypeError, W + "cameras must be float32"),
    (dict(device="cpu"), RuntimeError, W + "device must be a GPU"),
])
def test_triangulate_keypoints_refuses_before_any_launch(kw, error, text):
    from kasportsformer_amd import triangulate_keypoints
    kw = dict(kw)
    with pytest.raises(error) as e:
        triangulate_keypoints(kw.pop("keypoints", KP), kw.pop("cameras", CAMS), **kw)
    assert str(e.value).startswith(text), str(e.value)


K1 = np.zeros((5, 17, 3), np.float32)
CAM4, LENS5 = np.array([1500, 1500, 960, 540], np.float32), np.zeros(5, np.float32)
V = "undistort_keypoints: "


@pytest.mark.parametrize("kw,error,text", [
    (dict(iterations=-1), ValueError, V + "iterations must be in [0, 20]"),
    (dict(iterations=21), ValueError, V + "iterations must be in [0, 20]"),
    (dict(iterations=1.0), TypeError, V + "iterations must be an int"),
    (dict(keypoints=K1.tolist()), TypeError, V + "keypoints must be a numpy array or a torch tensor"),
    (dict(keypoints=K1.astype(np.float64)), TypeError, V + "keypoints must be float32"),
    (dict(keypoints=np.zeros((5, 17, 2), np.float32)), ValueError, V + "expected keypoints of [...,J,3]"),
    (dict(keypoints=np.zeros(3, np.float32)), ValueError, V + "expected keypoints of [...,J,3]"),
    (dict(camera=np.zeros(3, np.float32)), ValueError, V + "camera must be [4] (fx, fy, cx, cy) or [5, 4]"),
    (dict(camera=np.zeros((4, 4), np.float32)), ValueError, V + "camera must be [4] (fx, fy, cx, cy) or [5, 4]"),
    (dict(camera=CAM4.astype(np.float64)), TypeError, V + "camera must be float32"),
    (dict(distortion=np.zeros(4, np.float32)), ValueError, V + "distortion must be [5] (k1, k2, p1, p2, k3) or [5, 5]"),
    (dict(distortion=np.zeros((5, 4), np.float32)), ValueError, V + "distortion must be [5] (k1, k2, p1, p2, k3) or [5, 5]"),
    (dict(distortion=[0.0] * 5), TypeError, V + "distortion must be a numpy array or a torch tensor"),
    (dict(device="cpu"), RuntimeError, V + "device must be a GPU"),
])
def test_undistort_keypoints_refuses_before_any_launch(kw, error, text):
    from kasportsformer_amd import undistort_keypoints
    kw = dict(kw)
    with pytest.raises(error) as e:
        undistort_keypoints(kw.pop("keypoints", K1), kw.pop("camera", CAM4), kw.pop("distortion", LENS5), **kw)
    assert str(e.value).startswith(text), str(e.value)


def test_camera_row_and_the_parameters_as_the_entry_takes_them():
    from kasportsformer_amd import camera_row
    from kasportsformer_amd.triangulate import triangulate_params
    from tests.triangulate_ref import camera_row as ref_row
    R3, t = np.arange(9.0).reshape(3, 3), np.array([1.0, 2.0, 3.0])
    row = camera_row((1500, 1400, 960, 540), (-0.1, 0.05, 0.001, 0.002, 0.01), R3, t)
    assert row.dtype == np.float32 and row.shape == (21,) and np.array_equal(row, ref_row((1500, 1400, 960, 540), (-0.1, 0.05, 0.001, 0.002, 0.01), R3, t))
    assert row[:4].tolist() == [1500.0, 1400.0, 960.0, 540.0] and row[9:18].tolist() == list(range(9)) and row[18:].tolist() == [1.0, 2.0, 3.0]
    assert np.array_equal(camera_row((1, 2, 3, 4), None, R3, t)[4:9], np.zeros(5, np.float32))
    rows = camera_row(np.ones((6, 4)), np.zeros((6, 5)), np.tile(R3, (6, 1, 1)), np.tile(t, (6, 1)))
    assert rows.shape == (6, 21)
    for bad in (dict(intrinsics=(1, 2, 3)), dict(distortion=(0, 0, 0, 0)), dict(R=np.eye(4)), dict(t=(0, 0))):
        with pytest.raises(ValueError, match="camera_row: expected intrinsics"):
            camera_row(**{**dict(intrinsics=(1, 2, 3, 4), distortion=(0, 0, 0, 0, 0), R=R3, t=t), **bad})
    p = triangulate_params()
    assert (p.weighted, p.iterations, p.min_views, p.undistort_iterations) == (1, 4, 2, 5) and p.min_score == np.float32(0.3) and p.delta == 3.0
    p = triangulate_params(0, False, np.int64(8), 1, 16, 0)
    assert (p.min_score, p.weighted, p.iterations, p.delta, p.min_views, p.undistort_iterations) == (0.0, 0, 8, 1.0, 16, 0)
