"""The transformer surrogate families as one table (`graphs.FAMILIES`): what the package answers about every family is what it
answered before the families were folded into one block of `graphs.py` and one table row each (tests/golden/family_table.json, recorded on the
commit its generator names), and the table itself is sound.  Test-size twins only."""
import json
import os

import pytest

from i2v_amd import graphs, lib
from tests import make_family_table_fixture as mk

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "family_table.json")) as _fh:
    WANT = json.load(_fh)


def _json(value):
    return json.loads(json.dumps(value))


def test_the_fixture_covers_every_family():
    words = [f.word for f in graphs.FAMILIES]
    assert len(words) == len(set(words)) == 12
    assert {k.split("/")[0] for k in WANT["twins"]} == set(words) == set(WANT["refusals"]) == set(mk.BAD)
    assert sorted(WANT["twins"]) == sorted(f"{w}/{n}/{s}" for w, n, sides in mk.TWINS for s in sides)


@pytest.mark.parametrize("case", sorted(WANT["twins"]))
def test_twin_answers_what_it_answered(case):
    """Synthetic weights and packed arrays bit for bit (seeds 0 and 3), the key list, MACs, hooks, hook shapes, the planned bytes and
    the bytes of the ctypes config."""
    word, name, side = case.split("/")
    got, want = _json(mk.twin_record(name, int(side))), WANT["twins"][case]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], (case, field)
    fam = graphs.FAMILY_OF[type(graphs.build_tiny(name, (int(side),) * 2))]
    assert fam.word == word and fam.spec.__name__ == want["type"]


@pytest.mark.parametrize("word", sorted(WANT["refusals"]))
def test_refusals_keep_their_type_and_message(word):
    got, want = _json(mk.refusal_record(word)), WANT["refusals"][word]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], (word, field)


def test_resolvers_on_names_outside_every_family():
    got = {f"{fn}/{name}": mk._raised(getattr(graphs, fn), name) for fn in ("build", "build_surrogate", "build_tiny") for name in mk.RESOLVER_NAMES}
    assert _json(got) == WANT["resolvers"]
    assert WANT["resolvers"]["build/pit_s_224"][0] == "UnboundLocalError"        # (the reference's error for a name `build` does not know)


def test_help_text():
    assert mk.help_string() == WANT["help"]


def test_every_served_name_belongs_to_one_family():
    for fam in graphs.FAMILIES:
        assert fam.models is getattr(graphs, fam.word.upper() + "_MODELS")
        for name in fam.models:
            assert [f.word for f in graphs.FAMILIES if f.is_name(name)] == [fam.word], name
            assert type(graphs.build_surrogate(name)) is fam.spec, name
            assert (type(graphs.build(name)) is fam.spec) if fam.in_build else True
            assert type(graphs.build_tiny(name, fam.tiny_twin(name, (224, 224)).in_hw)) is fam.spec
    assert [f.word for f in graphs.FAMILIES if not f.in_build] == ["pit", "coat", "tnt"]


def test_every_family_has_its_prototypes():
    assert [f.word for f in graphs.FAMILIES if f.word not in lib.FAMILY_PROTOS] == []
    assert set(lib.FAMILY_PROTOS) == {f.word for f in graphs.FAMILIES}
    for fam in graphs.FAMILIES:
        assert f"i2v_{fam.word}_create" in lib.FAMILY_PROTOS[fam.word]
