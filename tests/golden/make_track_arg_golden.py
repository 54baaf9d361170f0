#!/usr/bin/env python3
"""Record what every refused call of tests/track_arg_cases.py raises and says (run ONCE, on the commit BEFORE a change to the argument handling of lift.py,
stream.py, tracked.py, smooth.py or bones.py).

    python tests/golden/make_track_arg_golden.py       # needs no device and no built library

Replays the table and writes track_arg_refusals.json: one record per case with the call, the case id, the exception's class name and its text.
tests/test_track_args_cpu.py holds every later commit to these records byte for byte, so the file is regenerated only when a message, an exception type or the
order of two checks is meant to change -- never to make that test pass.  Cases for a new surface are appended by running this on the commit that introduces it
and keeping every other record as it is (the script refuses to change one)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from tests import track_arg_cases as A  # noqa: E402


def main():
    lines = set()
    records = A.replay(lines)
    if os.path.exists(A.GOLDEN):
        old = {(r["call"], r["case"]): r for r in json.load(open(A.GOLDEN))}
        changed = [r for r in records if old.get((r["call"], r["case"]), r) != r]
        assert not changed, f"these records would change: {changed[:5]}"
    with open(A.GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in records) + "\n]\n")
    raises = A.raise_lines()
    missed = [r for r in raises if (r[0], r[1]) not in lines]
    print(f"wrote track_arg_refusals.json: {len(records)} cases, {len({(r['call'], r['message']) for r in records})} distinct messages, "
          f"{os.path.getsize(A.GOLDEN)} bytes; {len(raises)} raise statements, {len(missed)} not reached:")
    for m, line, text in missed:
        print(f"  {m}:{line}: {text[:120]}")


if __name__ == "__main__":
    main()
