"""Every refusal of kasf_match_workspace_bytes, kasf_match_pair_costs and kasf_match_groups (csrc/api_match.hip): code 2 (-2 from the byte count), the message
in kasf_last_error(), reached with null or bogus host pointers so that nothing is launched and no GPU is needed, the host buffers unchanged (tests/refusal_cases.py's
caller, table form and generated null / all_wrong / pair cases; the tables are this file's own).  Every message literal of api_match.hip is hit by some case.
Then the refusals of ``match_costs``, ``match_groups``, ``match_players`` and ``gather_matched``, all raised before any launch; and the C refusals once more
from a stand-alone C program under the address and undefined-behaviour sanitizers, against the library's host-sanitizer build, as a process of its own."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import refusal_cases as R

API = os.path.join(R.ROOT, "kasportsformer_amd", "csrc", "api_match.hip")
NAN, INF = float("nan"), float("inf")


class Match(C.Structure):        # kasf_match_params
    _fields_ = [("min_score", C.c_float), ("weighted", C.c_int32), ("cap", C.c_float), ("min_samples", C.c_int32), ("undistort_iterations", C.c_int32)]


def par(**kw):
    return Match(**{**dict(min_score=0.3, weighted=1, cap=50.0, min_samples=34, undistort_iterations=5), **kw})


def shape_cases(who, frames=True):
    out = [("cameras_small", dict(cameras=1), who + "cameras must be in [2, 16]"), ("cameras_big", dict(cameras=17), who + "cameras must be in [2, 16]"),
           ("rows_small", dict(rows=0), who + "rows must be in [1, 64]"), ("rows_big", dict(rows=65), who + "rows must be in [1, 64]")]
    if frames:
        out += [("frames_neg", dict(frames=-1), who + "frames must be in [0, 2^31 - 1]"), ("frames_big", dict(frames=2 ** 31), who + "frames must be in [0, 2^31 - 1]")]
    return out


W, P_, G_ = "match_workspace_bytes: ", "match_pair_costs: ", "match_groups: "
# (case, overrides, message) in the order of the entry's checks
PAIR_CASES = shape_cases(P_) + [
    ("joints", dict(joints=0), P_ + "joints must be >= 1"),
    ("samples_big", dict(frames=2 ** 30, joints=2), P_ + "frames * joints must stay below 2^31"),
    ("score_nan", dict(params=par(min_score=NAN)), P_ + "min_score must be finite"), ("score_inf", dict(params=par(min_score=INF)), P_ + "min_score must be finite"),
    ("weighted", dict(params=par(weighted=2)), P_ + "weighted must be 0 or 1"), ("weighted_neg", dict(params=par(weighted=-1)), P_ + "weighted must be 0 or 1"),
    ("cap_zero", dict(params=par(cap=0.0)), P_ + "cap must be finite and > 0"), ("cap_neg", dict(params=par(cap=-1.0)), P_ + "cap must be finite and > 0"),
    ("cap_nan", dict(params=par(cap=NAN)), P_ + "cap must be finite and > 0"), ("cap_inf", dict(params=par(cap=INF)), P_ + "cap must be finite and > 0"),
    ("min_samples", dict(params=par(min_samples=0)), P_ + "min_samples must be >= 1"),
    ("rounds_neg", dict(params=par(undistort_iterations=-1)), P_ + "undistort_iterations must be in [0, 20]"),
    ("rounds_big", dict(params=par(undistort_iterations=21)), P_ + "undistort_iterations must be in [0, 20]"),
    ("workspace_bytes", dict(workspace_bytes=20 * 3 * 25 - 1), P_ + "workspace_bytes is less than kasf_match_workspace_bytes asks for"),
    ("workspace_align", dict(workspace=R.OFF(4)), P_ + "workspace must be 8-byte aligned"),
]
GROUP_CASES = shape_cases(G_, frames=False) + [
    ("max_cost_zero", dict(max_cost=0.0), G_ + "max_cost must be finite and > 0"), ("max_cost_neg", dict(max_cost=-2.0), G_ + "max_cost must be finite and > 0"),
    ("max_cost_nan", dict(max_cost=NAN), G_ + "max_cost must be finite and > 0"), ("max_cost_inf", dict(max_cost=INF), G_ + "max_cost must be finite and > 0"),
    ("groups_small", dict(max_groups=0), G_ + "max_groups must be in [1, 64]"), ("groups_big", dict(max_groups=65), G_ + "max_groups must be in [1, 64]"),
]
ENTRIES = {
    "kasf_match_workspace_bytes": (dict(cameras=3, rows=5, frames=12), shape_cases(W)),
    "kasf_match_pair_costs": (dict(cameras=3, rows=5, frames=12, joints=17, params=par(), workspace_bytes=20 * 3 * 25), PAIR_CASES),
    "kasf_match_groups": (dict(cameras=3, rows=5, max_cost=15.0, max_groups=10), GROUP_CASES),
}


def entry(name):
    base, cases = ENTRIES[name]
    return (name, base, [(c, o) for c, o, _ in cases], ())


def library():
    lib = C.CDLL(R.LIB_PATH)
    lib.kasf_last_error.restype = C.c_char_p
    return lib


def replay(name):
    lib, said, e = library(), {}, entry(name)
    for cid, overrides, first in R.cases_of(e):
        code = R._call(lib, e[0], e[1], overrides)
        said[cid] = lib.kasf_last_error().decode()
        assert code == (-2 if name.endswith("bytes") else 2), f"{name} {cid}: code {code} ({said[cid]}): the call was not refused with 2"
        assert first is None or said[cid] == said[first], f"{name} {cid}: says {said[cid]!r}, not {said[first]!r}"
    return said


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_refusal_is_code_2_with_its_message(name):
    said = replay(name)
    for cid, _, message in ENTRIES[name][1]:
        assert said[cid] == message, cid
    nulls = {cid for cid in said if cid.startswith("null:")}
    want = {"kasf_match_workspace_bytes": set(),
            "kasf_match_pair_costs": {"null:keypoints", "null:camera_rows", "null:params", "null:cost", "null:samples", "null:workspace"},
            "kasf_match_groups": {"null:" + p for p in ("cost", "samples", "group", "members", "views", "group_cost", "count", "dropped")}}[name]
    assert nulls == want                                                 # no pointer of these entries may be NULL
    assert all(said[cid] == "null pointer argument" for cid in nulls)
    assert said["all_wrong"] == ENTRIES[name][1][0][2]


def test_a_refused_call_leaves_the_host_buffers_as_they_were():
    lib = library()
    lib.kasf_match_pair_costs.restype = lib.kasf_match_groups.restype = C.c_int
    buf = np.full(4096, 7.0, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for q in (par(cap=0.0), par(min_samples=0), par(weighted=3)):
        assert lib.kasf_match_pair_costs(p, 3, 5, C.c_int64(12), 17, p, C.byref(q), p, p, p, C.c_int64(1 << 20), None) == 2
    assert lib.kasf_match_pair_costs(p, 3, 5, C.c_int64(12), 17, p, C.byref(par()), p, p, p, C.c_int64(8), None) == 2       # the workspace is too small
    assert lib.kasf_match_pair_costs(p, 3, 65, C.c_int64(12), 17, p, C.byref(par()), p, p, p, C.c_int64(1 << 20), None) == 2
    assert lib.kasf_match_groups(p, p, 3, 5, C.c_float(15.0), 0, p, p, p, p, p, p, None) == 2
    assert lib.kasf_match_groups(p, p, 1, 5, C.c_float(15.0), 10, p, p, p, p, p, p, None) == 2
    assert (buf == 7.0).all()


def test_nothing_to_do_succeeds_without_a_launch_and_the_byte_count_is_the_stated_one():
    """frames == 0 returns 0 before it looks at a data pointer; the parameters are checked all the same."""
    lib = library()
    name, base = "kasf_match_pair_costs", ENTRIES["kasf_match_pair_costs"][0]
    nothing = {p: None for p in ("keypoints", "camera_rows", "cost", "samples", "workspace")}
    assert R._call(lib, name, {**base, "frames": 0, "workspace_bytes": 0}, nothing) == 0
    assert R._call(lib, name, {**base, "frames": 0, "params": par(cap=0.0)}, nothing) == 2
    assert R._call(lib, name, {**base, "frames": 0, "cameras": 1}, nothing) == 2
    for cameras, rows, frames in ((2, 1, 1), (3, 5, 256), (3, 5, 257), (7, 22, 18000), (16, 64, 2), (2, 3, 0)):
        want = 20 * ((frames + 255) // 256) * (cameras * (cameras - 1) // 2) * rows * rows
        assert R._call(lib, "kasf_match_workspace_bytes", dict(cameras=cameras, rows=rows, frames=frames), {}) == want


def test_every_message_of_the_file_has_a_case():
    text = re.sub(r"//[^\n]*", "", open(API).read())
    assert set(re.findall(r"^(?:int|int64_t) (kasf_\w+)\(", text, flags=re.M)) == set(ENTRIES)
    said = set().union(*(set(replay(name).values()) for name in ENTRIES))
    literals = [s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', text) if len(s) >= 8 and not s.endswith(".h") and not s.startswith("match_")]
    assert len(literals) >= 13
    missing = [s for s in literals if not any(s in m for m in said)]
    assert not missing, missing


def test_the_symbols_are_declared_in_the_header_exported_and_prototyped():
    from kasportsformer_amd import _lib
    assert [p for p, _, _ in R.PROTOS["kasf_match_workspace_bytes"][1]] == ["cameras", "rows", "frames"]
    assert [p for p, _, _ in R.PROTOS["kasf_match_pair_costs"][1]] == [
        "keypoints", "cameras", "rows", "frames", "joints", "camera_rows", "params", "cost", "samples", "workspace", "workspace_bytes", "stream"]
    assert [p for p, _, _ in R.PROTOS["kasf_match_groups"][1]] == [
        "cost", "samples", "cameras", "rows", "max_cost", "max_groups", "group", "members", "views", "group_cost", "count", "dropped", "stream"]
    lib = library()
    for name in ENTRIES:
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == len(R.PROTOS[name][1])
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    lib.kasf_version.restype = C.c_int
    assert lib.kasf_version() == 12 == _lib.ABI_VERSION                  # additive: the ABI version stays
    assert C.sizeof(_lib.KasfMatchParams) == C.sizeof(Match) == 20
    assert [(n, C.sizeof(t)) for n, t in _lib.KasfMatchParams._fields_] == [(n, C.sizeof(t)) for n, t in Match._fields_]
    header = open(os.path.join(R.ROOT, "include", "kasf.h")).read()
    body = re.search(r"typedef struct kasf_match_params \{(.*?)\} kasf_match_params;", header, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [n for n, _ in Match._fields_]
    mk = open(os.path.join(R.ROOT, "kasportsformer_amd", "csrc", "Makefile")).read()
    assert "k_match.hip" in mk and mk.count("api_match.hip") == 2 and "$(BUILD)/k_match.o: EXTRA += -Rpass-analysis=kernel-resource-usage" in mk


KP = np.zeros((3, 5, 4, 17, 3), np.float32)
CAMS = np.zeros((3, 21), np.float32)
COST, SAMPLES = np.zeros((3, 3, 5, 5), np.float32), np.zeros((3, 3, 5, 5), np.int32)


@pytest.mark.parametrize("who", ["match_costs", "match_players"])
@pytest.mark.parametrize("kw,error,text", [
    (dict(min_score="0.3"), TypeError, "min_score must be a number"),
    (dict(min_score=NAN), ValueError, "min_score must be finite"),
    (dict(cap=True), TypeError, "cap must be a number"),
    (dict(cap=INF), ValueError, "cap must be finite"),
    (dict(cap=0.0), ValueError, "cap must be > 0 pixels"),
    (dict(weighted=1), TypeError, "weighted must be a bool"),
    (dict(min_samples=0), ValueError, "min_samples must be in [1, 2147483647]"),
    (dict(min_samples=2.0), TypeError, "min_samples must be an int"),
    (dict(undistort_iterations=-1), ValueError, "undistort_iterations must be in [0, 20]"),
    (dict(undistort_iterations=21), ValueError, "undistort_iterations must be in [0, 20]"),
    (dict(undistort_iterations=5.0), TypeError, "undistort_iterations must be an int"),
    (dict(keypoints="kp"), TypeError, "keypoints must be a numpy array or a torch tensor"),
    (dict(keypoints=KP.astype(np.float64)), TypeError, "keypoints must be float32"),
    (dict(keypoints=[KP[0], KP[1].astype(np.float16), KP[2]]), TypeError, "keypoints[1] must be float32"),
    (dict(keypoints=[KP[0], KP[1, :, :3], KP[2]]), ValueError, "every camera's keypoints must have one N and one J"),
    (dict(keypoints=[KP[0], KP[1, 0], KP[2]]), ValueError, "expected every camera's keypoints as [P,N,J,3]"),
    (dict(keypoints=[KP[0]]), ValueError, "expected the keypoints of 2 to 16 cameras, got 1"),
    (dict(keypoints=np.zeros((17, 2, 1, 1, 3), np.float32)), ValueError, "expected the keypoints of 2 to 16 cameras, got 17"),
    (dict(keypoints=np.zeros((3, 65, 1, 1, 3), np.float32)), ValueError, "expected 1 to 64 rows per camera, got 65"),
    (dict(keypoints=np.zeros((3, 0, 1, 1, 3), np.float32)), ValueError, "expected 1 to 64 rows per camera, got 0"),
    (dict(keypoints=np.zeros((3, 5, 4, 17, 2), np.float32)), ValueError, "expected keypoints of [C,P,N,J,3]"),
    (dict(keypoints=np.zeros((3, 5, 4, 0, 3), np.float32)), ValueError, "expected keypoints of [C,P,N,J,3]"),
    (dict(keypoints=np.zeros((3, 5, 17, 3), np.float32)), ValueError, "expected keypoints of [C,P,N,J,3]"),
    (dict(cameras=np.zeros((3, 20), np.float32)), ValueError, "cameras must be [3, 21]"),
    (dict(cameras=np.zeros((2, 21), np.float32)), ValueError, "cameras must be [3, 21]"),
    (dict(cameras=np.zeros((3, 4, 21), np.float32)), ValueError, "cameras must be [3, 21]"),
    (dict(cameras=CAMS.tolist()), TypeError, "cameras must be a numpy array or a torch tensor"),
    (dict(cameras=CAMS.astype(np.float64)), TypeError, "cameras must be float32"),
    (dict(device="cpu"), RuntimeError, "device must be a GPU"),
])
def test_match_costs_and_match_players_refuse_before_any_launch(who, kw, error, text):
    import kasportsformer_amd as K_
    kw = dict(kw)
    with pytest.raises(error) as e:
        getattr(K_, who)(kw.pop("keypoints", KP), kw.pop("cameras", CAMS), **kw)
    assert str(e.value).startswith(who + ": " + text), str(e.value)


@pytest.mark.parametrize("who", ["match_groups", "match_players"])
@pytest.mark.parametrize("kw,error,text", [
    (dict(max_cost="15"), TypeError, "max_cost must be a number"),
    (dict(max_cost=NAN), ValueError, "max_cost must be finite"),
    (dict(max_cost=0.0), ValueError, "max_cost must be > 0 pixels"),
    (dict(max_groups=0), ValueError, "max_groups must be in [1, 64]"),
    (dict(max_groups=65), ValueError, "max_groups must be in [1, 64]"),
    (dict(max_groups=True), TypeError, "max_groups must be an int"),
])
def test_the_grouping_parameters_are_refused_before_any_launch(who, kw, error, text):
    import kasportsformer_amd as K_
    with pytest.raises(error) as e:
        K_.match_groups(COST, SAMPLES, **kw) if who == "match_groups" else K_.match_players(KP, CAMS, **kw)
    assert str(e.value).startswith(who + ": " + text), str(e.value)


@pytest.mark.parametrize("kw,error,text", [
    (dict(cost=COST.tolist()), TypeError, "cost must be a numpy array or a torch tensor"),
    (dict(cost=COST.astype(np.float64)), TypeError, "cost must be float32"),
    (dict(samples=SAMPLES.astype(np.int64)), TypeError, "samples must be int32"),
    (dict(cost=np.zeros((3, 2, 5, 5), np.float32)), ValueError, "expected cost of [C,C,P,P]"),
    (dict(cost=np.zeros((3, 3, 5, 4), np.float32)), ValueError, "expected cost of [C,C,P,P]"),
    (dict(cost=np.zeros((1, 1, 5, 5), np.float32)), ValueError, "expected cost of [C,C,P,P]"),
    (dict(cost=np.zeros((3, 3, 65, 65), np.float32)), ValueError, "expected cost of [C,C,P,P]"),
    (dict(samples=np.zeros((3, 3, 5, 4), np.int32)), ValueError, "samples must have the shape of cost"),
    (dict(device="cpu"), RuntimeError, "device must be a GPU"),
])
def test_match_groups_refuses_before_any_launch(kw, error, text):
    import kasportsformer_amd as K_
    kw = dict(kw)
    with pytest.raises(error) as e:
        K_.match_groups(kw.pop("cost", COST), kw.pop("samples", SAMPLES), **kw)
    assert str(e.value).startswith("match_groups: " + text), str(e.value)


def test_gather_matched_refuses_what_is_no_match_for_these_cameras():
    import torch
    import kasportsformer_amd as K_
    groups = K_.MatchGroups(*[torch.zeros((4, 2), dtype=torch.int32)] * 6)
    for bad in (None, groups, K_.MatchGroups(*[torch.zeros((4, 3), dtype=torch.int64)] * 6)):
        with pytest.raises(ValueError, match="gather_matched: match must be the result of match_players or match_groups for these 3 cameras"):
            K_.gather_matched(KP, bad)
    with pytest.raises(ValueError, match="gather_matched: expected keypoints of"):
        K_.gather_matched(KP[0], groups)


def test_the_parameters_as_the_entry_takes_them():
    from kasportsformer_amd.match import match_params
    p = match_params(17)
    assert (p.weighted, p.min_samples, p.undistort_iterations) == (1, 34, 5) and p.min_score == np.float32(0.3) and p.cap == 50.0
    p = match_params(3, 0, False, 1, np.int64(7), 0)
    assert (p.min_score, p.weighted, p.cap, p.min_samples, p.undistort_iterations) == (0.0, 0, 1.0, 7, 0)


DRIVER = r'''#include <math.h>
#include <stdio.h>
#include <string.h>
#include "kasf.h"
static int said(const char* want) { return strcmp(kasf_last_error(), want) == 0; }
int main(void) {
    static float f[1024];
    static int32_t i[1024];
    kasf_match_params p = {0.3f, 1, 50.0f, 34, 5};
    if (kasf_match_workspace_bytes(3, 5, 257) != 20 * 2 * 3 * 25) return 1;
    if (kasf_match_workspace_bytes(1, 5, 257) != -2 || !said("match_workspace_bytes: cameras must be in [2, 16]")) return 2;
    if (kasf_match_workspace_bytes(3, 65, 257) != -2 || kasf_match_workspace_bytes(3, 5, -1) != -2) return 3;
    if (kasf_match_pair_costs(f, 17, 5, 12, 17, f, &p, f, i, f, 1 << 20, 0) != 2) return 4;
    if (kasf_match_pair_costs(f, 3, 0, 12, 17, f, &p, f, i, f, 1 << 20, 0) != 2) return 5;
    if (kasf_match_pair_costs(f, 3, 5, (int64_t)1 << 31, 17, f, &p, f, i, f, 1 << 20, 0) != 2) return 6;
    if (kasf_match_pair_costs(f, 3, 5, 12, 0, f, &p, f, i, f, 1 << 20, 0) != 2) return 7;
    if (kasf_match_pair_costs(f, 3, 5, (int64_t)1 << 30, 2, f, &p, f, i, f, 1 << 20, 0) != 2 || !said("match_pair_costs: frames * joints must stay below 2^31")) return 8;
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, 0, f, i, f, 1 << 20, 0) != 2 || !said("null pointer argument")) return 9;
    kasf_match_params q = p;
    q.min_score = NAN;
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &q, f, i, f, 1 << 20, 0) != 2) return 10;
    q = p, q.weighted = 2;
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &q, f, i, f, 1 << 20, 0) != 2) return 11;
    q = p, q.cap = INFINITY;
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &q, f, i, f, 1 << 20, 0) != 2) return 12;
    q = p, q.min_samples = 0;
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &q, f, i, f, 1 << 20, 0) != 2) return 13;
    q = p, q.undistort_iterations = 21;
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &q, f, i, f, 1 << 20, 0) != 2) return 14;
    if (kasf_match_pair_costs(0, 3, 5, 0, 17, 0, &p, 0, 0, 0, 0, 0) != 0) return 15;                      /* no frames: nothing to do */
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &p, f, 0, f, 1 << 20, 0) != 2) return 16;               /* samples */
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &p, f, i, f, 1499, 0) != 2 || !said("match_pair_costs: workspace_bytes is less than kasf_match_workspace_bytes asks for")) return 17;
    if (kasf_match_pair_costs(f, 3, 5, 12, 17, f, &p, f, i, (char*)f + 4, 1 << 20, 0) != 2 || !said("match_pair_costs: workspace must be 8-byte aligned")) return 18;
    if (kasf_match_groups(f, i, 1, 5, 15.0f, 10, i, i, i, f, i, i, 0) != 2) return 19;
    if (kasf_match_groups(f, i, 3, 65, 15.0f, 10, i, i, i, f, i, i, 0) != 2) return 20;
    if (kasf_match_groups(f, i, 3, 5, 0.0f, 10, i, i, i, f, i, i, 0) != 2 || !said("match_groups: max_cost must be finite and > 0")) return 21;
    if (kasf_match_groups(f, i, 3, 5, NAN, 10, i, i, i, f, i, i, 0) != 2) return 22;
    if (kasf_match_groups(f, i, 3, 5, 15.0f, 65, i, i, i, f, i, i, 0) != 2 || !said("match_groups: max_groups must be in [1, 64]")) return 23;
    if (kasf_match_groups(f, i, 3, 5, 15.0f, 10, i, i, i, f, i, 0, 0) != 2 || !said("null pointer argument")) return 24;
    for (int k = 0; k < 1024; ++k)
        if (f[k] != 0.0f || i[k] != 0) return 25;
    printf("ok\n");
    return 0;
}
'''


def test_the_refusals_in_a_program_of_their_own_under_address_and_ub_sanitizers(tmp_path):
    """`make asan` builds the host code of the C entries, api_match.hip among them, with -fsanitize=address,undefined; a C program built with the same runtime
    walks the refusals as its own process.  Nothing is preloaded."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    clang = "/opt/rocm/lib/llvm/bin/clang"
    if not (os.path.exists(hipcc) and os.path.exists(clang)):
        pytest.skip("ROCm clang not available")
    csrc = os.path.join(R.ROOT, "kasportsformer_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-j", "4", "all", "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    src, exe = tmp_path / "refuse.c", tmp_path / "refuse"
    src.write_text(DRIVER)
    libdir = os.path.join(R.ROOT, "kasportsformer_amd")
    r = subprocess.run([clang, "-std=c99", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-shared-libsan",
                        "-I" + os.path.join(R.ROOT, "include"), str(src), "-o", str(exe), "-L" + libdir, "-l:libkasf_hip_asan.so", "-lm", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib/clang/22/lib/linux"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
