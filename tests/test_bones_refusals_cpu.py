"""Every refusal of the four entry points in csrc/api_bones.hip: code 2, the message in kasf_last_error(), reached with null or bogus host pointers so that
nothing is launched and no GPU is needed (tests/refusal_cases.py's caller, table form and generated null / all_wrong / pair cases).  Every message literal of
api_bones.hip is hit by some case, and every entry it defines has a row."""
import ctypes as C
import os
import re

from tests import refusal_cases as R

API = os.path.join(R.ROOT, "kasportsformer_amd", "csrc", "api_bones.hip")
_SIZES = [("N", dict(N=-1)), ("P", dict(P=-1)), ("N_big", dict(N=2 ** 31))]
_WINDOW = [("window_0", dict(window=0)), ("window_big", dict(window=2 ** 20 + 1))]
_TRACKED = [("streams", dict(streams=0)), ("track_slots", dict(track_slots=65)), ("R", dict(R=0)), ("rows_mode", dict(rows_mode=2)),
            ("bits", dict(streams=2 ** 30, R=4))]
# (entry, a base that passes every check but the pointers', [(case, overrides)], parameters that may be NULL)
ENTRIES = [
    ("kasf_bone_median", dict(N=4, P=1), _SIZES, ("counts",)),
    ("kasf_bone_apply", dict(N=4, P=1, per_track=1), _SIZES + [("alias", dict(out=R.SAME("poses")))], ()),
    ("kasf_bone_push", dict(K=1, S=2, window=4), [("K", dict(K=3)), ("S", dict(S=-1, K=0)), ("no_ids", dict(slots=None))] + _WINDOW, ("slots",)),
    ("kasf_bone_tracked", dict(streams=1, track_slots=2, rows_mode=0, R=1, window=4), _TRACKED + _WINDOW, ("row_slot",)),
]
MESSAGES = {
    "N": "bones: N and P must be >= 0", "P": "bones: N and P must be >= 0", "N_big": "bones: N must be below 2^31",
    "alias": "bones: out and poses must be distinct arrays", "K": "bones: need 0 <= K <= S", "S": "bones: need 0 <= K <= S",
    "no_ids": "bones: without slot ids the call covers every slot (K == S)", "window_0": "bones: window must be in [1, 2^20]",
    "window_big": "bones: window must be in [1, 2^20]", "streams": "bones: streams must be >= 1", "track_slots": "bones: track_slots must be in [1, 64]",
    "R": "bones: R must be >= 1", "rows_mode": "bones: rows_mode must be KASF_ROWS_PERSONS or KASF_ROWS_TRACKS",
    "bits": "bones: streams * R and streams * track_slots must fit 32 bits",
}


def replay():
    lib = C.CDLL(R.LIB_PATH)
    lib.kasf_last_error.restype = C.c_char_p
    records = []
    for entry in ENTRIES:
        said = {}
        for cid, overrides, first in R.cases_of(entry):
            code = R._call(lib, entry[0], entry[1], overrides)
            said[cid] = lib.kasf_last_error().decode()
            assert code == 2, f"{entry[0]} {cid}: code {code} ({said[cid]}): the call was not refused with 2"
            assert first is None or said[cid] == said[first], f"{entry[0]} {cid}: says {said[cid]!r}, not {said[first]!r}"
            records.append((entry[0], cid, said[cid]))
    return records


def test_every_refusal_is_code_2_with_its_message():
    records = replay()
    for entry, cid, message in records:
        if cid in MESSAGES:
            assert message == MESSAGES[cid], (entry, cid, message)
        elif cid.startswith("null:"):
            assert message == "null pointer argument", (entry, cid, message)
    # a pointer that may be NULL is not refused for it: the generated cases skip it, and each entry has null cases for all the others
    for name, _, _, nullable in ENTRIES:
        pointers = [p for p, _, ptr in R.PROTOS[name][1] if ptr and p != "stream" and p not in nullable]
        assert {cid for e, cid, _ in records if e == name and cid.startswith("null:")} == {f"null:{p}" for p in pointers}
    # the median needs neither poses nor a scratch for N = 0, and the shared table no offsets: with the other pointers null they get as far as the null refusal
    lib = C.CDLL(R.LIB_PATH)
    lib.kasf_last_error.restype = C.c_char_p
    assert R._call(lib, "kasf_bone_median", dict(N=0, P=1, poses=None, scratch=None, lengths=None), {}) == 2
    assert lib.kasf_last_error().decode() == "null pointer argument"
    assert R._call(lib, "kasf_bone_apply", dict(N=4, P=0, per_track=0, offsets=None, out=None), {}) == 2
    assert lib.kasf_last_error().decode() == "null pointer argument"
    # what does nothing returns 0 before it looks at a pointer
    assert R._call(lib, "kasf_bone_median", dict(N=4, P=0), {p: None for p in ("poses", "offsets", "scratch", "lengths", "counts")}) == 0
    assert R._call(lib, "kasf_bone_apply", dict(N=0, P=1), {p: None for p in ("poses", "offsets", "lengths", "out")}) == 0
    assert R._call(lib, "kasf_bone_push", dict(K=0, S=2, window=4), {p: None for p in ("poses", "slots", "len", "cnt", "out")}) == 0


def test_every_entry_and_every_message_of_the_file_has_a_case():
    text = re.sub(r"//[^\n]*", "", open(API).read())
    defined = set(re.findall(r"^(?:int|int64_t) (kasf_\w+)\(", text, flags=re.M))
    assert defined == {e[0] for e in ENTRIES} and len(defined) == 4
    said = {m for _, _, m in replay()}
    literals = [s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', text) if len(s) >= 8 and not s.endswith(".h")]
    assert len(literals) >= 5
    missing = [s for s in literals if not any(s in m for m in said)]
    assert not missing, missing
