"""Every refusal of the C entry points in csrc/api_video.hip and csrc/api_ops.hip, held to what the library said before they were split out of engine.hip:
tests/refusal_cases.py is the table of refused calls, tests/golden/refusals.json what each of them returned and left in kasf_last_error().  A refusal returns before
any device call, so nothing is launched and no GPU is needed."""
import json
import os
import re

from tests import refusal_cases as R

CSRC = os.path.join(R.ROOT, "kasportsformer_amd", "csrc")
API_FILES = ("api_video.hip", "api_ops.hip", "api_check.h")


def test_refusals_match_the_golden_byte_for_byte():
    golden = json.load(open(R.GOLDEN))
    now = R.replay()                                   # asserts on its own that no case reaches a launch and that a pair case says what its first half says
    assert [(g["entry"], g["case"]) for g in golden] == [(n["entry"], n["case"]) for n in now], "the table and the golden list different cases"
    wrong = [(g, n) for g, n in zip(golden, now) if g != n]
    assert not wrong, f"{len(wrong)} refusals changed, the first: {wrong[0]}"
    assert all(g["code"] != 0 for g in golden)


def test_every_entry_and_every_message_has_a_case():
    golden = json.load(open(R.GOLDEN))
    text = "".join(open(os.path.join(CSRC, f)).read() for f in API_FILES)
    text = re.sub(r"//[^\n]*", "", text)
    # every entry point defined in the two files
    defined = set(re.findall(r"^(?:int|int64_t) (kasf_\w+)\(", text, flags=re.M))
    assert len(defined) >= 60
    assert defined == {e[0] for e in R.ENTRIES} == {g["entry"] for g in golden}
    # every message in the three files (a whole one, or the part behind "<entry>: ") is one that some case was given
    said = {g["message"] for g in golden} | {m for _, m, _ in R.UNREACHABLE}
    literals = [s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', text) if len(s) >= 8 and not s.endswith(".h")]
    literals = [s for s in literals if s not in ("k_loss7's LDS at the largest clip", "kasf.h and kernels.h disagree on the size of a statistics buffer")]   # static_assert
    assert len(literals) >= 100
    missing = [s for s in literals if not any(s in m for m in said)]
    assert not missing, missing
    # what no case can reach is listed with its reason, and is at most 5 % of the refusals
    hit = {(g["entry"], g["message"]) for g in golden}
    assert all(reason and (entry, message) not in hit for entry, message, reason in R.UNREACHABLE)
    assert len(R.UNREACHABLE) * 20 <= len(hit) + len(R.UNREACHABLE)
