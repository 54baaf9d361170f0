"""The refusals of the track, slot and stream arguments of lift.py, stream.py, tracked.py, smooth.py and bones.py, held to what they raised and said before
their argument handling moved into one shared module: tests/track_arg_cases.py is the table of refused calls, tests/golden/track_arg_refusals.json the exception
class and the text of each.  Every call is refused before the library is loaded or a device is touched, so no GPU is needed.  Also: the device side's one
statement of the tracked-row rule, csrc/tracked_rows.h, is the only one and every object file is rebuilt when it changes."""
import json

from tests import track_arg_cases as A


def test_refusals_match_the_golden_byte_for_byte_and_reach_every_raise():
    golden = json.load(open(A.GOLDEN))
    lines = set()
    now = A.replay(lines)                              # asserts on its own that every call is refused, by a message of the call's own
    assert [(g["call"], g["case"]) for g in golden] == [(n["call"], n["case"]) for n in now], "the table and the golden list different cases"
    wrong = [(g, n) for g, n in zip(golden, now) if g != n]
    assert not wrong, f"{len(wrong)} refusals changed, the first: {wrong[0]}"
    # every raise statement of the modules is reached by some case, or listed with its reason: at most 10 % of them
    raises = A.raise_lines()
    assert len(raises) >= 60
    missed = [(m, text) for m, line, text in raises if (m, line) not in lines]
    listed = lambda m, text: any(m == lm and piece in text for lm, piece, _ in A.UNREACHED)      # noqa: E731
    seen = {m: sum(1 for f, _ in lines if f == m) for m in A.MODULES}
    assert not [r for r in missed if not listed(*r)], (seen, [r for r in missed if not listed(*r)])
    assert all(reason and any(m == lm and piece in text for m, text in missed) for lm, piece, reason in A.UNREACHED), "a listed raise is reached, or gone"
    assert len(A.UNREACHED) * 10 <= len(raises)


def test_the_row_rule_has_one_home_and_every_object_depends_on_it():
    import glob
    import os
    csrc = os.path.join(A.ROOT, "kasportsformer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    rules = [ln for ln in mk.splitlines() if ln.startswith("$(BUILD)/%.o:") or ln.startswith("build_asan/%.o:")]
    assert len(rules) == 2 and all("tracked_rows.h" in ln for ln in rules)
    text = {os.path.basename(f): open(f).read() for f in glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip"))}
    assert [f for f, t in text.items() if "#define KASF_ROWS_PERSONS" in t] == ["tracked_rows.h"]
    assert sorted(f for f, t in text.items() if "tracked_row(" in t) == ["k_bones.hip", "k_smooth.hip", "k_stream_track.hip", "tracked_rows.h"]
    assert [f for f, t in text.items() if "__syncthreads_or(hit" in t] == ["tracked_rows.h"]
