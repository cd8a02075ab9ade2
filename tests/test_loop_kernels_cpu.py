"""The loop-kernel case table (tests/loop_cases.py) on the host simulation against the float64 references, the checks that keep a case
from passing vacuously, and the refusals of the C entries."""
import pytest
import torch

from tests import loop_cases as lc
from tests.hostsim_util import hostsim_engine
from tests.make_loop_fixtures import load

E32 = load()


def test_the_fixture_covers_the_table():
    assert set(E32) == {c.id for c in lc.CASES}


@pytest.mark.parametrize("case", lc.CASES, ids=[c.id for c in lc.CASES])
def test_case_on_the_host_simulation(case):
    lc.check(case, lc.run(hostsim_engine(), case), E32[case.id], report=print)


# ---- input sanity -------------------------------------------------------------------------------------------------------------
def _rel_change(case, drop):
    """max over the outputs both have of |ref - ref without `drop`| / |ref| (2-norms)."""
    full, less = lc.evaluate(case, raw=True), lc.evaluate(case, drop=drop, raw=True)
    worst = 0.0
    for name, (kind, want) in full.items():
        if kind != "exact" and name in less:
            worst = max(worst, float((want - less[name][1]).norm() / want.norm()))
    return worst


MASKED = [c for c in lc.CASES if c.kw.get("mask")]


@pytest.mark.parametrize("case", MASKED, ids=[c.id for c in MASKED])
def test_the_mask_gates_a_fair_share_and_changes_the_reference(case):
    inp = lc.inputs(case)
    for name in ("a1", "a2") if case.op == "head" and not case.kw["fused"] else ("a1",) if case.op == "head" else ("a",):
        share = float((inp[name] > 0).float().mean())
        assert 0.2 <= share <= 0.8, (case.id, name, share)
    assert _rel_change(case, "mask") > 0.05, case.id


@pytest.mark.parametrize("drop,select", [
    ("bias", lambda c: c.op == "head" and c.kw["bias"]),
    ("second", lambda c: c.op == "head" and not c.kw["fused"]),
    ("momentum", lambda c: c.op == "gp" and c.kw["mom"]),
    ("segments", lambda c: c.op in ("ilaf", "tapd") and c.kw["fps"] < c.kw["frames"]),
])
def test_every_ingredient_changes_the_reference(drop, select):
    """Without the bias, the second pooled feature, the momentum or the segment boundary the reference moves by more than 5 % of its
    norm: a kernel that ignored the ingredient could not pass."""
    cases = [c for c in lc.CASES if select(c)]
    assert cases
    for c in cases:
        if c.kw.get("shape", (0,))[-1] == 224:      # (the grid-cap case repeats a small case's arithmetic on 4.8 M elements)
            continue
        assert _rel_change(c, drop) > 0.05, (c.id, drop, _rel_change(c, drop))


def test_planted_edges_are_in_the_inputs():
    z = lc.inputs(lc.BY_ID["cos-zero-row"])["a"]
    assert not bool(z[1].any()) and bool(z[0].any())
    x = lc.inputs(lc.BY_ID["tap_sign-n5000"])["x"]
    bits = x.view(torch.int32)
    assert int((bits == 0).sum()) > 100 and int((bits == -2 ** 31).sum()) > 100      # +0.0 and -0.0
    a = lc.inputs(lc.BY_ID["tapd-D37-f6-seg2-pad3-m1a0"])["a"]
    assert int((a == 0).sum()) > 10 and int((a < 0).sum()) > 10
    c = lc.inputs(lc.BY_ID["compose-layout0"])
    eps = torch.tensor(c["eps"], dtype=torch.float32)
    s = c["u"] + c["d"].clamp(-c["eps"], c["eps"])
    assert int((c["d"] == eps).sum()) >= 2 and int((c["d"] == -eps).sum()) >= 2 and int((s == 1).sum()) >= 2 and int((s == 0).sum()) >= 2
    assert int((c["d"].abs() > eps).sum()) > 50 and int((s > 1).sum()) >= 2 and int((s < 0).sum()) >= 2
    labels = [int(v) for cs in lc.CASES if cs.op == "head" for v in lc.inputs(cs)["labels"]]
    assert 0 in labels and 299 in labels and 256 in labels and 1 in labels
    mv = lc.inputs(lc.BY_ID["ttmix-D3-w0.3"])["moves"]
    assert int(mv.min()) < -5 and int(mv.max()) > 5
    k = lc.inputs(lc.BY_ID["dwconv-2x3x4x6x5-axis3-k15"])["taps"]
    assert float((k - k.flip(0)).abs()[:7].min()) > 0.05                              # no tap equals its mirror image


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_entry():
    eng = hostsim_engine()
    thunks, keep = lc.refusals(eng)
    assert len(thunks) > 40
    for label, name, thunk in thunks:
        assert thunk() != 0, label
        text = eng.capi.i2v_last_error().decode()
        assert text.startswith(name + ":"), (label, text)
    del keep
