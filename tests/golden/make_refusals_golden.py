#!/usr/bin/env python3
"""Record what every refused call of tests/refusal_cases.py returns and says (run ONCE, on a build of the commit BEFORE a change to the entry points).

    make -C kasportsformer_amd/csrc && python tests/golden/make_refusals_golden.py       # or KASF_LIB=<another build>; needs no device

Replays the table against the library and writes refusals.json: one record per case with the entry, the case id, the return code and the text of
kasf_last_error().  tests/test_refusals_cpu.py holds every later build to these records byte for byte, so the file is regenerated only when a message, a code or
the order of two checks is meant to change -- never to make that test pass.  New cases for a new entry point are appended by running this on the build that
introduces it and keeping the records of every other entry as they are (the script refuses to change one)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests import refusal_cases as R  # noqa: E402


def main():
    records = R.replay()
    if os.path.exists(R.GOLDEN):
        old = {(r["entry"], r["case"]): r for r in json.load(open(R.GOLDEN))}
        changed = [r for r in records if old.get((r["entry"], r["case"]), r) != r]
        assert not changed, f"these records would change: {changed[:5]}"
    with open(R.GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in records) + "\n]\n")
    pairs = {(r["entry"], r["message"]) for r in records}
    print(f"wrote refusals.json: {len(records)} cases of {len(R.ENTRIES)} entries, {len(pairs)} distinct (entry, message) pairs, {os.path.getsize(R.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
