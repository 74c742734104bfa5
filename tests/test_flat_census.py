"""CPU-only: the census of the flat engine's compiled kernels (tests/flat_census.py) is complete and stands on what it says it stands on.
Every instantiation loik_flat_inst.hpp lists (k_flat1 at both NA) and the four builds of k_flat have a recipe, and no recipe predicts a
kernel that is not compiled; the carrier trees are accepted by the flat schedule with the lane counts, depths and round counts written
beside them; and the oracle alone converges on every instance of every recipe's batch, so that the GPU comparison of
tests/test_flat_instantiations.py compares converged solves."""
import collections

import numpy as np
import pytest

import flat_census as C
from helpers import caterpillar_parents, comb_parents, random_tree, star_parents, tree_from_parents


def test_every_compiled_instantiation_has_one_recipe():
    want = C.listed()
    assert len(want) == 18 + 2 * 14 + 4
    got = collections.Counter(C.predicted(rc) for rc in C.RECIPES + C.UNREACHABLE_RECIPES)
    # (the two builds nothing launches are written down like the others: k_flat<double, 16, LOG>, see flat_census.UNREACHABLE_RECIPES)
    assert {C.predicted(rc) for rc in C.UNREACHABLE_RECIPES} == {("k_flat", 16, False), ("k_flat", 16, True)}
    assert set(got) >= want, ("compiled kernels without a recipe", sorted(C.inst_id(i) for i in want - set(got)))
    assert set(got) <= want, ("recipes that predict a kernel nobody compiles", sorted(C.inst_id(i) for i in set(got) - want))
    assert max(got.values()) == 1, ("two recipes for one kernel", [C.inst_id(i) for i, n in got.items() if n > 1])


def test_recipes_use_the_carriers_their_family_asks_for():
    for rc in C.RECIPES:
        inst = C.predicted(rc)
        if inst[:2] == ("k_flat1", 16):
            assert rc.carrier in ("caterpillar(33,17)", "comb(64,17)"), rc
        elif inst[0] == "k_flat1":
            assert rc.carrier in ("comb(33,11)", "star(33)", "talos44"), rc
        elif inst[0] == "k_flat2":
            assert rc.carrier in ("comb(32,11)", "star(17)", "talos32"), rc
    deep = [(rc.carrier, C.predicted(rc)[2]) for rc in C.RECIPES if C.predicted(rc)[:2] == ("k_flat1", 16)]
    assert set(deep) == {(c, s) for c in ("caterpillar(33,17)", "comb(64,17)") for s in (False, True)}, "both depth-17 carriers, sliced and not"


def test_carrier_constructions():
    assert comb_parents(8, 4) == [0, 0, 1, 1, 1, 1, 1, 6, 7]
    assert caterpillar_parents(7, 4) == [0, 0, 1, 1, 3, 3, 5, 5]
    assert star_parents(3) == [0, 0, 0, 0]
    # tree_from_parents draws the joints as random_tree does: the same generator, the same draws in the same order -- random_tree's
    # own generator, once it has drawn the shape, continues with exactly them
    a = random_tree(6, 21)
    rng = np.random.default_rng(6)
    path = [0]
    for i in range(1, 22):
        while len(path) > 1 and rng.random() < 0.35:
            path.pop()
        path.append(i)
    t = tree_from_parents(a.parents, 6)
    r = np.random.default_rng(6)
    assert int(t.jtype[1]) == int(r.integers(1, 9))     # (a fresh generator: the first joint's type is its first draw)
    assert int(a.jtype[1]) == int(rng.integers(1, 9))   # (random_tree: the first draw after the shape's)
    b, c = tree_from_parents(comb_parents(21, 5), 3), tree_from_parents(comb_parents(21, 5), 3)
    assert np.array_equal(b.jtype, c.jtype) and np.array_equal(b.placement, c.placement) and np.array_equal(b.axis, c.axis)
    assert set(np.unique(b.jtype[1:])) <= set(range(1, 9))
    R = np.asarray(b.placement)[1:, :9].reshape(-1, 3, 3)
    assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.abs(np.asarray(b.placement)[1:, 9:]).max() <= 0.4


@pytest.mark.parametrize("seed,nb,kw,want", [
    (6, 21, {}, (2885, 1050, 111.37704152, 22.598808241)),
    (12, 31, dict(branch_prob=0.3), (9493, 2050, 163.129509089, 32.329191834)),
    (9, 28, dict(branch_prob=0.45, all_types=False), (6769, 857, 143.193042642, 28.0)),
    (15, 60, dict(branch_prob=0.45), (65333, 8698, 306.517777313, 66.036408726))])
def test_random_tree_draws_what_it_always_drew(seed, nb, kw, want):
    """random_tree shares its joint draw with tree_from_parents: trees the suite uses, by checksums taken before the two were joined"""
    m = random_tree(seed, nb, **kw)
    idx = np.arange(nb + 1)
    assert (int(np.dot(idx, m.parents)), int(np.dot(idx, m.jtype))) == want[:2]
    assert abs(float(np.abs(m.placement).sum()) - want[2]) < 1e-8 and abs(float(np.abs(m.axis).sum()) - want[3]) < 1e-8


@pytest.mark.parametrize("name", list(C.CARRIER_TABLE))
def test_carriers_are_what_the_table_says(name):
    nb, G, depth, nanc, njmp, nscan, kernel, na = C.CARRIER_TABLE[name]
    model = C.model_of(name)
    fs = C.schedule_of(name)     # (asserts that the flat schedule accepts the tree)
    assert model.njoints - 1 == nb
    assert (fs["G"], int(fs["depth"].max()), fs["nanc"], fs["njmp"], fs["nscan"]) == (G, depth, nanc, njmp, nscan)
    assert C.flat_kind(fs["G"], fs["nanc"]) == kernel
    assert (C.FLAT_NA_SMALL if fs["nanc"] <= C.FLAT_NA_SMALL else C.FLAT_MAXA) == na
    if name.startswith("comb"):
        assert fs["size"][0] == nb and list(model.parents[2:nb - depth + 2]) == [1] * (nb - depth)
    if name.startswith("star"):
        assert np.all(fs["size"][:nb] == 1)
    if name == "comb(64,17)":    # no unused lane: every helper lane is a leaf of the tree
        assert fs["helper"].sum() > 0 and np.all(fs["size"][fs["helper"].astype(bool)] == 1)
    assert C.deepest_joint(model) == nb and fs["size"][nb - 1] == 1 and fs["depth"][nb - 1] == depth


def test_talos_carriers_are_shallow():
    for name, kernel in (("talos32", "k_flat2"), ("talos44", "k_flat1")):
        fs = C.schedule_of(name)
        assert fs["nanc"] <= C.FLAT_NA_SMALL and C.flat_kind(fs["G"], fs["nanc"]) == kernel


def _workloads():
    seen = {}
    for rc in C.RECIPES + C.UNREACHABLE_RECIPES:
        seen.setdefault((rc.carrier, C.batch_of(rc), rc.hm, rc.mur == 1), rc)
    return seen


@pytest.mark.parametrize("key", list(_workloads()), ids=lambda k: "%s-B%d-hm%d-%s" % (k[0], k[1], k[2], "osqp" if k[3] else "decades"))
def test_oracle_converges_on_every_batch(key):
    """the condition on the inputs of the GPU census: within the end-to-end cap of 400 iterations at 1e-6 the oracle converges on every
    instance and flags none infeasible"""
    rc = _workloads()[key]
    wl = C.workload(rc)
    out = C.oracle_end_to_end(wl, rc.mur == 1)
    assert out["converged"].all() and not out["primal_infeasible"].any() and out["iters"].max() < C.END_TO_END["max_iter"] - 1
    if rc.sliced:   # (a slice is 5 iterations: somebody must live to the second one)
        assert out["iters"].max() > 5
    assert wl["num_eq_c"] == (2 if rc.hm == 3 and rc.carrier.startswith("comb") else 1)
    assert np.abs(wl["v_ref"]).min() > 0


@pytest.mark.parametrize("name", list(C.CARRIER_TABLE))
def test_oracle_converges_on_the_edge_shapes(name):
    out = C.oracle_end_to_end(C.plain_workload(name), False)
    assert out["converged"].all() and not out["primal_infeasible"].any() and out["iters"].max() < C.END_TO_END["max_iter"] - 1


def _well_posed(wl, osqp, B, tol):
    from test_engines import FIELDS, SCALARS
    assert C.FIELD_NAMES == FIELDS
    for k in C.K_ITERATIONS:
        for b in range(0, B, C.SAMPLE_EVERY):
            sens = C.oracle_sensitivity(wl, osqp, k, b, SCALARS)
            assert sens <= tol / 10, (k, b, sens)


@pytest.mark.parametrize("key", list(_workloads()), ids=lambda k: "%s-B%d-hm%d-%s" % (k[0], k[1], k[2], "osqp" if k[3] else "decades"))
def test_comparisons_are_well_posed(key):
    """The second condition on the inputs, again by the oracle alone: at the instances and iteration counts where the GPU census compares
    fields with a fixed bound (1e-9, OSQP's rule 1e-8), the oracle's own fields move by no more than a tenth of that bound when its
    inputs are perturbed by a relative 1e-15.  Ten is the margin tests/test_qp_optimum_gpu.py gives an engine over the oracle's own
    error; an instance that fails this compares roundings, not kernels (flat_census.oracle_sensitivity).  A batch that fails gets
    another seed, never another bound."""
    rc = _workloads()[key]
    _well_posed(C.workload(rc), rc.mur == 1, C.batch_of(rc), 1e-8 if rc.mur == 1 else 1e-9)


@pytest.mark.parametrize("name", list(C.CARRIER_TABLE))
def test_comparisons_on_the_edge_shapes_are_well_posed(name):
    _well_posed(C.plain_workload(name), False, 130, 1e-9)
