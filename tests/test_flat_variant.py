"""CPU-only: which instantiation <SLICED, HM, LOG, MUR> of k_flat2 / k_flat1 a launch runs (loikb_flat_variant; flat_variant in
loik_amd/csrc/loik_host.hip) -- all 96 inputs against the table written out here, and against the instantiation lists of
loik_amd/csrc/loik_flat_inst.hpp: every variant returned is listed, every listed instance is returned for some input."""
import itertools
import os
import re

import pytest

from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT2, FLAT1 = 2, 1

# (kind, mur, logging, hm) -> (SLICED or None = as wanted, HM, LOG, MUR), every row written out
TABLE = {
    # k_flat2, OSQP's rule: the reference weight as it is, sliced only with h I; logging does not matter
    (FLAT2, 1, 0, 0): (None, 0, False, 1), (FLAT2, 1, 0, 1): (False, 1, False, 1), (FLAT2, 1, 0, 2): (False, 2, False, 1), (FLAT2, 1, 0, 3): (False, 3, False, 1),
    (FLAT2, 1, 1, 0): (None, 0, False, 1), (FLAT2, 1, 1, 1): (False, 1, False, 1), (FLAT2, 1, 1, 2): (False, 2, False, 1), (FLAT2, 1, 1, 3): (False, 3, False, 1),
    # k_flat2, the lazily populated table: h I whatever hm says
    (FLAT2, 2, 0, 0): (None, 0, False, 2), (FLAT2, 2, 0, 1): (None, 0, False, 2), (FLAT2, 2, 0, 2): (None, 0, False, 2), (FLAT2, 2, 0, 3): (None, 0, False, 2),
    (FLAT2, 2, 1, 0): (None, 0, False, 2), (FLAT2, 2, 1, 1): (None, 0, False, 2), (FLAT2, 2, 1, 2): (None, 0, False, 2), (FLAT2, 2, 1, 3): (None, 0, False, 2),
    # k_flat2, decade steps: the SolverInfo lists unsliced, a diagonal weight as a general one; else as wanted
    (FLAT2, 0, 1, 0): (False, 0, True, 0), (FLAT2, 0, 1, 1): (False, 2, True, 0), (FLAT2, 0, 1, 2): (False, 2, True, 0), (FLAT2, 0, 1, 3): (False, 3, True, 0),
    (FLAT2, 0, 0, 0): (None, 0, False, 0), (FLAT2, 0, 0, 1): (None, 1, False, 0), (FLAT2, 0, 0, 2): (None, 2, False, 0), (FLAT2, 0, 0, 3): (None, 3, False, 0),
    # k_flat1, OSQP's rule: unsliced, a diagonal weight as a general one
    (FLAT1, 1, 0, 0): (False, 0, False, 1), (FLAT1, 1, 0, 1): (False, 2, False, 1), (FLAT1, 1, 0, 2): (False, 2, False, 1), (FLAT1, 1, 0, 3): (False, 3, False, 1),
    (FLAT1, 1, 1, 0): (False, 0, False, 1), (FLAT1, 1, 1, 1): (False, 2, False, 1), (FLAT1, 1, 1, 2): (False, 2, False, 1), (FLAT1, 1, 1, 3): (False, 3, False, 1),
    # k_flat1 has no lazily populated table: mur 2 as mur 0
    (FLAT1, 2, 1, 0): (False, 0, True, 0), (FLAT1, 2, 1, 1): (False, 2, True, 0), (FLAT1, 2, 1, 2): (False, 2, True, 0), (FLAT1, 2, 1, 3): (False, 3, True, 0),
    (FLAT1, 2, 0, 0): (None, 0, False, 0), (FLAT1, 2, 0, 1): (None, 1, False, 0), (FLAT1, 2, 0, 2): (None, 2, False, 0), (FLAT1, 2, 0, 3): (None, 3, False, 0),
    (FLAT1, 0, 1, 0): (False, 0, True, 0), (FLAT1, 0, 1, 1): (False, 2, True, 0), (FLAT1, 0, 1, 2): (False, 2, True, 0), (FLAT1, 0, 1, 3): (False, 3, True, 0),
    (FLAT1, 0, 0, 0): (None, 0, False, 0), (FLAT1, 0, 0, 1): (None, 1, False, 0), (FLAT1, 0, 0, 2): (None, 2, False, 0), (FLAT1, 0, 0, 3): (None, 3, False, 0),
}
INPUTS = list(itertools.product((FLAT2, FLAT1), range(4), (0, 1), (0, 1), range(3)))   # kind, hm, sliced, logging, mur


def listed_instances():
    """{kind: set of (SLICED, HM, LOG, MUR)} as LOIKB_FLAT2_INSTANCES / LOIKB_FLAT1_INSTANCES_NA list them"""
    text = open(os.path.join(ROOT, "loik_amd", "csrc", "loik_flat_inst.hpp")).read().replace("\\\n", " ")
    out = {}
    for kind, macro, pat in ((FLAT2, "LOIKB_FLAT2_INSTANCES(X)", r"X\((true|false), (\d), (true|false), (\d)\)"),
                             (FLAT1, "LOIKB_FLAT1_INSTANCES_NA(X, NA)", r"X\(NA, (true|false), (\d), (true|false), (\d)\)")):
        body = next(line for line in text.split("\n") if line.startswith("#define " + macro))
        out[kind] = {(s == "true", int(hm), lg == "true", int(mur)) for s, hm, lg, mur in re.findall(pat, body)}
    assert len(out[FLAT2]) == 18 and len(out[FLAT1]) == 14
    return out


def test_every_input_against_the_table():
    assert len(INPUTS) == 96 and len(TABLE) == 48
    for kind, hm, sliced, logging, mur in INPUTS:
        want = TABLE[(kind, mur, logging, hm)]
        want = (bool(sliced) if want[0] is None else want[0],) + want[1:]
        assert capi.flat_variant(kind, hm, sliced, logging, mur) == want, (kind, hm, sliced, logging, mur)


def test_variants_and_instantiation_lists_coincide():
    listed = listed_instances()
    returned = {FLAT2: set(), FLAT1: set()}
    for kind, hm, sliced, logging, mur in INPUTS:
        returned[kind].add(capi.flat_variant(kind, hm, sliced, logging, mur))
    for kind in (FLAT2, FLAT1):
        assert returned[kind] <= listed[kind], ("not instantiated", returned[kind] - listed[kind])
        assert listed[kind] <= returned[kind], ("dead instantiations", listed[kind] - returned[kind])


def test_argument_errors():
    for bad in ((0, 0, 0, 0, 0), (3, 0, 0, 0, 0), (2, 4, 0, 0, 0), (2, -1, 0, 0, 0), (1, 0, 0, 0, 3), (1, 0, 0, 0, -1)):
        with pytest.raises(capi.LoikError):
            capi.flat_variant(*bad)
