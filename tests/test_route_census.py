"""Which launch sequence every kind of handle takes through the on-chip engines: the handles of tests/golden/make_route_census.py,
replayed and compared with the record of the commit before run_tail was split by engine (tests/golden/route_census_parent.json).
The record is not to be made anew for a change of the dispatch's form: a difference is a change of behaviour."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_route_census", os.path.join(GOLDEN, "make_route_census.py"))
census = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(census)

with open(os.path.join(GOLDEN, "route_census_parent.json")) as _f:
    PARENT = json.load(_f)


def test_the_record_covers_every_handle():
    assert set(PARENT) == set(census.CASES)
    for name, rec in PARENT.items():
        assert len(rec["iters"]) == 2 and len(rec["plan"]) == 2 and len(rec["stats"]) == 2, name
        assert rec["stats"][0] and rec["stats"][1], name   # (fields that did not repeat on the parent were dropped, never all)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(census.CASES))
def test_route_census(name):
    got, want = census.record(name), PARENT[name]
    print(name, got["stats"], got["iters"])
    assert got["iters"] == want["iters"], "the sum of the iteration counts differs: the arithmetic changed"
    for k in range(2):
        assert {f: got["stats"][k][f] for f in want["stats"][k]} == want["stats"][k], "solve %d" % k
        if want["plan"][k] is not None:
            assert got["plan"][k] == want["plan"][k], "solve %d" % k
