"""The planner's decisions over a fixed catalogue of graphs, against the recorded ones (tests/golden/plan_trace.txt, written by
tests/make_plan_trace_fixture.py): which 3x3 -> pointwise pairs, fast-pathway blocks and shortcut pairs are admitted or refused and
why, and which launches are hoisted to the side stream, after and before which.  Every fusing and hoisting pass of csrc/i2v_tune.cpp
asks one read/write-set analysis; an operand forgotten there, or a pass that asks it the wrong question, moves a line here."""
from tests import make_plan_trace_fixture as fixture


def test_plan_decisions_match_the_recorded_trace():
    with open(fixture.FIXTURE) as f:
        want = f.read().splitlines()
    for tag in ("[i2v fuse]", "[i2v fastblock]", "[i2v scpair]", "[i2v overlap]"):           # the record itself covers every pass ...
        assert any(l.startswith(tag) for l in want), tag
    assert any(l.startswith("[i2v fuse]") and "other_reader=1" in l for l in want)           # ... and refusals of both kinds of pair
    assert any(l.startswith("[i2v scpair]") and ("dependent=1" in l or "other_reader=1" in l) for l in want)
    got = fixture.trace()
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}: planned {g!r}, recorded {w!r}"
