"""The binding hands the C library what it handed it before its device / host pairs became one body each: the calls recorded
from the tree (tests/binding_calls.py: a stand-in library, no GPU) equal tests/golden/binding_calls.json, which the same
recorder wrote at the commit before that change -- function names, every scalar with its Python type, every array's dtype,
shape, contiguity and bytes, the ValueErrors, and the layout of what the methods return."""
import json
import os

import binding_calls


def _lines(case):
    out = ["  call %d: %s" % (n, c[0]) + "".join("\n    [%d] %s" % (i, a) for i, a in enumerate(c[1:], 1)) for n, c in enumerate(case["calls"])]
    res = case["result"]
    out += ["  result %s: %s" % (k, v) for k, v in res.items()] if isinstance(res, dict) else ["  result: %s" % (res,)]
    return "\n".join(out).split("\n")


def test_calls_equal_the_recording(golden_dir):
    with open(os.path.join(golden_dir, "binding_calls.json")) as f:
        want = json.load(f)
    got = json.loads(binding_calls.dumps(binding_calls.record()))
    assert [c["case"] for c in got] == [c["case"] for c in want]
    assert len(want) > 150 and len({c["calls"][0][0] for c in want if c["calls"]}) >= 70      # both forms of every pair
    diffs = []
    for g, w in zip(got, want):
        if g != w:
            gl, wl = _lines(g), _lines(w)
            rows = ["%s\n      recorded: %s" % (a, b) for a, b in zip(gl, wl) if a != b]
            if len(gl) != len(wl):
                rows.append("  %d lines, recorded %d" % (len(gl), len(wl)))
            diffs.append(g["case"] + "\n" + "\n".join(rows))
    assert not diffs, "%d of %d cases differ from the recording:\n%s" % (len(diffs), len(want), "\n".join(diffs))
