"""Every refusal of kasf_tracks_refine (csrc/api_refine.hip): code 2, the message in kasf_last_error(), reached with null or bogus host pointers so that nothing
is launched and no GPU is needed (tests/refusal_cases.py's caller, table form and generated null / all_wrong / pair cases; the table is this file's own).  Every
message literal of api_refine.hip is hit by some case.  Then the refusals of ``refine_tracks``, all raised before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import refusal_cases as R

API = os.path.join(R.ROOT, "kasportsformer_amd", "csrc", "api_refine.hip")
NAN, INF = float("nan"), float("inf")


class Refine(C.Structure):       # kasf_refine_params
    _fields_ = [("min_score", C.c_float), ("max_gap", C.c_int32), ("radius", C.c_int32), ("weights", C.c_float * 33)]


def refine(min_score=0.3, max_gap=15, radius=2, **w):
    """Weights 1, 0.5, 0.25 and garbage above the radius, which is ignored; w: w1=..., w0=... replace single entries."""
    table = [1.0, 0.5, 0.25] + [NAN] * 30
    for k, v in w.items():
        table[int(k[1:])] = v
    return Refine(min_score, max_gap, radius, (C.c_float * 33)(*table))


_WEIGHT = "tracks_refine: weights[0 .. radius] must be finite, not negative and at most 1e6"
# (case, overrides, message) in the order of the entry's checks
CASES = [
    ("J_0", dict(J=0), "tracks_refine: J must be in [1, 256]"), ("J_big", dict(J=257), "tracks_refine: J must be in [1, 256]"),
    ("C_0", dict(C=0), "tracks_refine: C must be in [1, 4]"), ("C_big", dict(C=5), "tracks_refine: C must be in [1, 4]"),
    ("P", dict(P=-1), "tracks_refine: P and N must be >= 0"), ("N", dict(N=-1), "tracks_refine: P and N must be >= 0"),
    ("gap_neg", dict(params=refine(max_gap=-1)), "tracks_refine: max_gap must be in [0, 64]"),
    ("gap_big", dict(params=refine(max_gap=65)), "tracks_refine: max_gap must be in [0, 64]"),
    ("radius_neg", dict(params=refine(radius=-1)), "tracks_refine: radius must be in [0, 32]"),
    ("radius_big", dict(params=refine(radius=33)), "tracks_refine: radius must be in [0, 32]"),
    ("score_nan", dict(params=refine(min_score=NAN)), "tracks_refine: min_score must be finite"),
    ("score_inf", dict(params=refine(min_score=-INF)), "tracks_refine: min_score must be finite"),
    ("w_nan", dict(params=refine(w1=NAN)), _WEIGHT), ("w_inf", dict(params=refine(w2=INF)), _WEIGHT), ("w_neg", dict(params=refine(w1=-0.5)), _WEIGHT),
    ("w_big", dict(params=refine(w2=2e6)), _WEIGHT), ("w0_nan", dict(params=refine(w0=NAN)), _WEIGHT),
    ("w0_zero", dict(params=refine(w0=0.0)), "tracks_refine: weights[0] must be > 0"),
]
ENTRY = ("kasf_tracks_refine", dict(N=4, P=1, J=17, C=2, has_score=1, params=refine()), [(c, o) for c, o, _ in CASES], ("state",))


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
    assert nulls == {"null:x", "null:offsets", "null:params", "null:out"}          # state may be NULL
    assert all(said[cid] == "null pointer argument" for cid in nulls)
    assert said["all_wrong"] == "tracks_refine: J must be in [1, 256]"
    # what does nothing returns 0 before it looks at a data pointer; the parameters are checked all the same
    lib = library()
    nothing = {p: None for p in ("x", "offsets", "out", "state")}
    assert R._call(lib, ENTRY[0], {**ENTRY[1], "P": 0}, nothing) == 0
    assert R._call(lib, ENTRY[0], {**ENTRY[1], "N": 0}, nothing) == 0
    assert R._call(lib, ENTRY[0], {**ENTRY[1], "N": 0, "params": refine(max_gap=65)}, nothing) == 2
    # entries above the radius are ignored: the base's are NaN
    assert R._call(lib, ENTRY[0], {**ENTRY[1], "N": 0, "params": refine(radius=0, w1=-1.0)}, nothing) == 0


def test_every_message_of_the_file_has_a_case():
    text = re.sub(r"//[^\n]*", "", open(API).read())
    assert set(re.findall(r"^(?:int|int64_t) (kasf_\w+)\(", text, flags=re.M)) == {ENTRY[0]}
    said = set(replay().values())
    literals = [s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', text) if len(s) >= 8 and not s.endswith(".h")]
    assert len(literals) >= 7
    missing = [s for s in literals if not any(s in m for m in said)]
    assert not missing, missing


def test_the_ctypes_struct_matches_the_header():
    from kasportsformer_amd import _lib
    assert C.sizeof(_lib.KasfRefineParams) == C.sizeof(Refine) == 4 * 36
    assert [(n, C.sizeof(t)) for n, t in _lib.KasfRefineParams._fields_] == [(n, C.sizeof(t)) for n, t in Refine._fields_]


TRACK = np.zeros((5, 17, 3), np.float32)


@pytest.mark.parametrize("kw,error,text", [
    (dict(min_score="0.3"), TypeError, "refine_tracks: min_score must be a number"),
    (dict(min_score=NAN), ValueError, "refine_tracks: min_score must be finite"),
    (dict(max_gap=-1), ValueError, "refine_tracks: max_gap"),
    (dict(max_gap=65), ValueError, "refine_tracks: max_gap"),
    (dict(max_gap=1.5), TypeError, "refine_tracks: max_gap"),
    (dict(sigma=0.0), ValueError, "refine_tracks: sigma must be in [1e-3, 1e3] frames"),
    (dict(sigma=NAN), ValueError, "refine_tracks: sigma must be in [1e-3, 1e3] frames"),
    (dict(sigma="2"), TypeError, "refine_tracks: sigma must be a number of frames or None"),
    (dict(radius=33), ValueError, "refine_tracks: radius"),
    (dict(radius=-1), ValueError, "refine_tracks: radius"),
    (dict(sigma=None, radius=3), ValueError, "refine_tracks: sigma=None is the gap fill alone"),
    (dict(score=1), TypeError, "refine_tracks: score must be a bool"),
    (dict(return_state=1), TypeError, "refine_tracks: return_state must be a bool"),
    (dict(tracks=np.zeros((5, 17), np.float32)), ValueError, "refine_tracks: expected tracks of [N,J,Ct]"),
    (dict(tracks=np.zeros((5, 17, 3), np.float64)), TypeError, "refine_tracks:"),
    (dict(tracks=np.zeros((5, 257, 3), np.float32)), ValueError, "refine_tracks: need J in [1, 256]"),
    (dict(tracks=np.zeros((5, 17, 6), np.float32)), ValueError, "refine_tracks: need J in [1, 256] and Ct - 1 in [1, 4]"),
    (dict(tracks=np.zeros((5, 17, 5), np.float32), score=False), ValueError, "refine_tracks: need J in [1, 256] and Ct in [1, 4]"),
    (dict(tracks=[TRACK, np.zeros((2, 16, 3), np.float32)]), ValueError, "refine_tracks: every track must have the same [J,Ct]"),
    (dict(offsets=[0, 6]), ValueError, "refine_tracks: offsets must be integers [P+1]"),
    (dict(offsets=[0, 3, 2, 5]), ValueError, "refine_tracks: offsets must be integers [P+1]"),
    (dict(tracks=np.zeros((2, 2, 5, 17, 3), np.float32)), ValueError, "refine_tracks: expected [N,J,Ct] or [P,N,J,Ct]"),
])
def test_refine_tracks_refuses_before_any_launch(kw, error, text):
    from kasportsformer_amd import refine_tracks
    kw = dict(kw)
    with pytest.raises(error) as e:
        refine_tracks(kw.pop("tracks", TRACK), **kw)
    assert str(e.value).startswith(text), str(e.value)


def test_default_radius_and_weights():
    from kasportsformer_amd.refine import refine_params
    from tests.refine_ref import weights
    for sigma, radius, want in ((2.0, None, 6), (0.5, None, 2), (20.0, None, 32), (2.0, 4, 4), (None, None, 0), (3.0, 0, 0)):
        p = refine_params(0.3, 15, sigma, radius)
        w, r = weights(sigma, radius)
        assert p.radius == r == want and p.max_gap == 15
        assert np.array_equal(np.array(p.weights[:], np.float32).view(np.uint32), w.view(np.uint32)) and w[0] == 1.0
