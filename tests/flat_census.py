"""The census of the flat engine's compiled kernels: one recipe per instantiation, shared by tests/test_flat_census.py (CPU: the table is
complete, the carriers are what they are said to be, the oracle converges on every recipe's batch) and tests/test_flat_instantiations.py
(GPU: every recipe against the oracle, and the launch is the predicted kernel).

A recipe is a launch described by its inputs -- a carrier tree, the kind of reference weight, time slices or not, logging or not, the
rule that moves mu, and where needed an environment switch -- that the host's own rules (flat_kind, flat_variant, launch_flat_kernel in
loik_amd/csrc/loik_host.hip) turn into ONE instantiation of k_flat2 / k_flat1 / k_flat.  Which one is computed here from
capi.flat_schedule and capi.flat_variant, never written down beside the recipe: a recipe that stops landing on its kernel shows."""
import collections
import functools
import re

import numpy as np

import loik_amd
from loik_amd import capi
import helpers
from helpers import FIXTURE, caterpillar_parents, comb_parents, star_parents, tree_from_parents
from oracle import ref
from test_flat_variant import FLAT1, FLAT2, listed_instances

FLAT_NA_SMALL, FLAT_MAXA = 10, 16   # (loik_flat.hpp)

# ---- the carrier trees: name -> (constructor, parents); shapes by construction (helpers.comb_parents / caterpillar_parents / star_parents)
_SHAPES = {
    "star(17)": star_parents(17), "comb(32,11)": comb_parents(32, 11), "comb(32,12)": comb_parents(32, 12), "comb(17,17)": comb_parents(17, 17),
    "caterpillar(24,17)": caterpillar_parents(24, 17), "star(33)": star_parents(33), "comb(33,11)": comb_parents(33, 11),
    "comb(33,12)": comb_parents(33, 12), "caterpillar(33,17)": caterpillar_parents(33, 17), "comb(64,17)": comb_parents(64, 17),
}
# what the flat schedule makes of each: nb, G, depth, nanc, njmp, nscan, kernel, NA -- written out, checked against capi.flat_schedule
# by tests/test_flat_census.py::test_carriers_are_what_the_table_says
CARRIER_TABLE = {
    "star(17)":           (17, 32, 1, 1, 0, 1, "k_flat2", 10),    # smallest flat robot of two lanes per joint, no ancestors, no jump rounds
    "comb(32,11)":        (32, 32, 11, 10, 4, 6, "k_flat2", 10),  # last depth k_flat2 takes; no unused lane; largest subtree exactly 32
    "comb(32,12)":        (32, 32, 12, 11, 4, 6, "k_flat", 16),   # one deeper: the other kernel
    "comb(17,17)":        (17, 32, 17, 16, 5, 5, "k_flat", 16),   # a pure chain at both depth limits (16 ancestors, 5 jump rounds)
    "caterpillar(24,17)": (24, 32, 17, 16, 5, 5, "k_flat", 16),   # deep, with helper lanes
    "star(33)":           (33, 64, 1, 1, 0, 1, "k_flat1", 10),    # smallest k_flat1 robot
    "comb(33,11)":        (33, 64, 11, 10, 4, 6, "k_flat1", 10),  # last NA = 10 depth
    "comb(33,12)":        (33, 64, 12, 11, 4, 6, "k_flat1", 16),  # first NA = 16 depth
    "caterpillar(33,17)": (33, 64, 17, 16, 5, 6, "k_flat1", 16),  # helper lanes among the free ones
    "comb(64,17)":        (64, 64, 17, 16, 5, 7, "k_flat1", 16),  # no unused lane: every helper is a leaf; largest subtree 64
}
CARRIERS = list(CARRIER_TABLE) + ["talos32", "talos44"]


# (seeds: the joints' draw per carrier, and further down the batches' -- chosen on the CPU, by the ORACLE alone: it converges on every
#  instance of every recipe's batch within the end-to-end cap and flags none infeasible, and where fields are compared after k iterations
#  its own answer is well posed: tests/test_flat_census.py::test_oracle_converges_on_every_batch, ::test_comparisons_are_well_posed)
MODEL_SEEDS = dict({c: 40 + k for k, c in enumerate(_SHAPES)}, **{"comb(32,11)": 58, "comb(33,11)": 50})


@functools.lru_cache(maxsize=None)
def model_of(name):
    if name in ("talos32", "talos44"):
        return loik_amd.builtin_model(name)
    return tree_from_parents(_SHAPES[name], MODEL_SEEDS[name], name=name)


@functools.lru_cache(maxsize=None)
def schedule_of(name):
    fs = capi.flat_schedule(model_of(name).parents)
    assert fs is not None, (name, capi.lib().loikb_last_error())
    return fs


def flat_kind(G, nanc, split=True):
    """flat_kind() of loik_host.hip for an fp64 handle whose tree the flat schedule takes: the kernel's name"""
    if not split:
        return "k_flat"
    if G == 32 and nanc <= FLAT_NA_SMALL:
        return "k_flat2"
    return "k_flat1" if G == 64 else "k_flat"


# ---- the recipes ----------------------------------------------------------------------------------------------------------------
# carrier; hm: 0 = h I (h != 1), 1 = diagonal, 2 = general symmetric, 3 = per link; sliced; logging; mur: 0 = decade steps from the table
# (LOIKB_FLAT_BUILD=0), 1 = OSQP's rule (mu_update_strat = 1), 2 = the lazily populated table (LOIKB_FLAT_BUILD=1, LOIKB_FLAT_WINDOW=0,1);
# env: further switches (LOIKB_FLAT_SPLIT=0 for k_flat on a tree k_flat2 would take)
Recipe = collections.namedtuple("Recipe", "carrier hm sliced logging mur env", defaults=((),))
C32, S17, T32 = "comb(32,11)", "star(17)", "talos32"
C33, S33, T44 = "comb(33,11)", "star(33)", "talos44"
K33, C64 = "caterpillar(33,17)", "comb(64,17)"
ONE_LANE = (("LOIKB_FLAT_SPLIT", "0"),)
RECIPES = [
    # (a star's joints do not interact: under a weight shared by the links an instance is at rounding level after six iterations -- no
    #  star where an instance must live to its second time slice or to a change of mu, and none under OSQP's rule, whose quotient of two
    #  residuals is ill posed there: oracle_sensitivity below)
    # k_flat2<10, ..>: 18
    Recipe(S17, 0, False, False, 0), Recipe(C32, 0, True, False, 0),
    Recipe(C32, 1, False, False, 0), Recipe(C32, 1, True, False, 0), Recipe(S17, 2, False, False, 0), Recipe(C32, 2, True, False, 0),
    Recipe(C32, 3, False, False, 0), Recipe(C32, 3, True, False, 0),
    Recipe(C32, 0, False, True, 0), Recipe(S17, 1, False, True, 0), Recipe(C32, 3, False, True, 0),   # (logging: a diagonal weight goes as a general one)
    Recipe(C32, 0, False, False, 1), Recipe(C32, 0, True, False, 1), Recipe(C32, 1, False, False, 1), Recipe(T32, 2, False, False, 1),
    Recipe(T32, 3, False, False, 1),
    Recipe(T32, 0, False, False, 2), Recipe(C32, 0, True, False, 2),
    # k_flat1<10, ..>: 14
    Recipe(S33, 0, False, False, 0), Recipe(C33, 0, True, False, 0), Recipe(C33, 1, False, False, 0), Recipe(T44, 1, True, False, 0),
    Recipe(S33, 2, False, False, 0), Recipe(C33, 2, True, False, 0), Recipe(C33, 3, False, False, 0), Recipe(C33, 3, True, False, 0),
    Recipe(C33, 0, False, True, 0), Recipe(S33, 1, False, True, 0), Recipe(C33, 3, False, True, 0),
    Recipe(C33, 0, False, False, 1), Recipe(T44, 1, False, False, 1), Recipe(C33, 3, False, False, 1),   # (OSQP's rule: diagonal as general too)
    # k_flat1<16, ..>: 14, on the two depth-17 carriers in turn
    Recipe(K33, 0, False, False, 0), Recipe(C64, 0, True, False, 0), Recipe(C64, 1, False, False, 0), Recipe(K33, 1, True, False, 0),
    Recipe(K33, 2, False, False, 0), Recipe(C64, 2, True, False, 0), Recipe(C64, 3, False, False, 0), Recipe(K33, 3, True, False, 0),
    Recipe(C64, 0, False, True, 0), Recipe(K33, 2, False, True, 0), Recipe(C64, 3, False, True, 0),
    Recipe(K33, 0, False, False, 1), Recipe(C64, 2, False, False, 1), Recipe(K33, 3, False, False, 1),
    # k_flat<double, 10, LOG>: 2 (launch_flat_kernel's last branch: NA = 10 when nanc <= 10, LOG = the handle's logging; h I only)
    Recipe(C32, 0, False, False, 0, ONE_LANE), Recipe(S17, 0, False, True, 0, ONE_LANE),
]
# k_flat<double, 16, LOG>: compiled, selected by flat_kind() for a 17..32-joint tree with more than 10 ancestors -- and never launched.
# flat_lds_bytes<double, 16> is 27.2 KB of row buffers before any instance's own block (2 x 17 rows of W / Dinv, 16 rows of products):
# five wavefronts per CU, and the plan (make_plan in loik_host.hip) gives a tree to k_flat from six.  Such a handle says "no k_flat:
# constraint blocks leave too few wavefronts per CU in LDS" and solves on the level-by-level engines.  The census keeps the two builds
# in sight: the launches that WOULD run them are written down like recipes, and tests/test_flat_instantiations.py asserts on the device
# that the plan refuses them (the day it does not, that test fails and the two builds need recipes) and compares what runs instead.
UNREACHABLE_RECIPES = [Recipe("comb(32,12)", 0, False, False, 0), Recipe("caterpillar(24,17)", 0, False, True, 0)]
NO_FLAT_ENGINE = "no k_flat: constraint blocks leave too few wavefronts per CU in LDS"
# the four builds of k_flat the host launches, written out (launch_flat_kernel in loik_host.hip: `auto* kernel = S->opt.logging ? ...`)
K_FLAT_BUILDS = {("k_flat", 10, False), ("k_flat", 10, True), ("k_flat", 16, False), ("k_flat", 16, True)}


def predicted(rc):
    """the instantiation the host's rules make of a recipe: ("k_flat2" | "k_flat1", NA, SLICED, HM, LOG, MUR) or ("k_flat", NA, LOG)"""
    fs = schedule_of(rc.carrier)
    kind = flat_kind(fs["G"], fs["nanc"], split=dict(rc.env).get("LOIKB_FLAT_SPLIT", "1") != "0")
    na = FLAT_NA_SMALL if fs["nanc"] <= FLAT_NA_SMALL else FLAT_MAXA
    if kind == "k_flat":
        assert rc.hm == 0 and not rc.sliced and rc.mur == 0, "k_flat takes h I, unsliced, decade steps from the table"
        return (kind, na, bool(rc.logging))
    assert kind == "k_flat2" or rc.mur != 2, "the lazily populated table is k_flat2's"
    return (kind, na) + capi.flat_variant(FLAT2 if kind == "k_flat2" else FLAT1, rc.hm, rc.sliced, rc.logging, rc.mur)


def listed():
    """every compiled instantiation, as loik_flat_inst.hpp lists them (k_flat1 at both NA) plus k_flat's four"""
    inst = listed_instances()
    out = {("k_flat2", FLAT_NA_SMALL) + v for v in inst[FLAT2]}
    out |= {("k_flat1", na) + v for na in (FLAT_NA_SMALL, FLAT_MAXA) for v in inst[FLAT1]}
    return out | K_FLAT_BUILDS


def launched_kernel(carrier):
    """the flat kernel a default handle of the carrier runs: the CARRIER_TABLE's, or None where that is the NA = 16 build of k_flat"""
    kernel, na = CARRIER_TABLE[carrier][6:8]
    return None if (kernel, na) == ("k_flat", FLAT_MAXA) else kernel


def inst_id(inst):
    if inst[0] == "k_flat":
        return "k_flat<double,%d,%s>" % (inst[1], "log" if inst[2] else "nolog")
    return "%s<%d,%s,hm%d,%s,mur%d>" % (inst[0], inst[1], "sliced" if inst[2] else "plain", inst[3], "log" if inst[4] else "nolog", inst[5])


def is_sliced(inst):
    return inst[0] != "k_flat" and inst[2]


def mur_of(inst):
    return 0 if inst[0] == "k_flat" else inst[5]


# ---- a recipe's launch: environment, constructor arguments, workload, the oracle's answer -----------------------------------------
ENV_NAMES = ("LOIKB_LEAN", "LOIKB_FLAT", "LOIKB_FLAT_SPLIT", "LOIKB_FLAT_SLICE", "LOIKB_LEAN_WG_PER_CU", "LOIKB_LEAN_KLO", "LOIKB_LEAN_DECADES",
             "LOIKB_LEAN_ADAPT", "LOIKB_FLAT_BUILD", "LOIKB_FLAT_WINDOW", "LOIKB_FLAT_SMALL_BATCH", "LOIKB_FLAT_MIN_BATCH", "LOIKB_FLAT_ORDER")


def environment(rc):
    # (one wavefront per CU and 700 instances: instances wait, so a slice of 5 iterations really parks them)
    env = dict(LOIKB_FLAT_SLICE="5", LOIKB_LEAN_WG_PER_CU="1") if rc.sliced else dict(LOIKB_FLAT_SLICE="0")
    env.update(dict(LOIKB_FLAT_BUILD="1", LOIKB_FLAT_WINDOW="0,1") if rc.mur == 2 else dict(LOIKB_FLAT_BUILD="0"))
    env.update(dict(rc.env))
    return env


def batch_of(rc):
    return 700 if rc.sliced else 130


def deepest_joint(model):
    depth = np.zeros(model.njoints, int)
    for i in range(1, model.njoints):
        depth[i] = depth[int(model.parents[i])] + 1
    return int(np.flatnonzero(depth == depth.max())[-1])   # (the last of the deepest: a leaf, also on a star)


H_DIAG = np.diag([0.4, 1.5, 0.7, 3.0, 0.2, 2.2])                    # (tests/test_engines.py::test_flat_engine_with_a_diagonal_reference_weight)
V_REF = np.array([0.02, -0.01, 0.03, 0.05, -0.04, 0.01])            # H_ref v_ref != 0: the reference term's subtree sums too


def reference_weight(hm):
    if hm == 0:
        return 0.7 * np.eye(6)           # h != 1: h is read
    if hm == 2:
        Q = np.linalg.qr(np.random.default_rng(4).normal(size=(6, 6)))[0]
        H = Q @ H_DIAG @ Q.T
        return 0.5 * (H + H.T)
    return H_DIAG                        # (hm 3: the shared weight SolveInit gets before UpdateReferences replaces it link by link)


# the batches' seeds: 300, or per (carrier, B, hm, OSQP's rule?) the first one above it that meets the two conditions on the inputs
DEFAULT_SEED = 300
WORKLOAD_SEEDS = {
    ("comb(32,11)", 700, 3, False): 303, ("comb(33,11)", 130, 3, False): 306, ("comb(33,11)", 700, 3, False): 317, ("comb(33,11)", 700, 2, False): 302,
    ("talos32", 130, 2, True): 301, ("talos32", 130, 3, True): 302, ("talos32", 130, 0, False): 302, ("star(33)", 130, 0, False): 303,
    ("talos44", 700, 1, False): 305, ("comb(64,17)", 130, 3, False): 304, ("comb(64,17)", 130, 2, True): 301,
}


def seed_of(carrier, B, hm, osqp):
    return WORKLOAD_SEEDS.get((carrier, B, hm, bool(osqp)), DEFAULT_SEED)


@functools.lru_cache(maxsize=None)
def _workload(carrier, B, hm, plain, seed):
    model = model_of(carrier)
    link = deepest_joint(model)
    if hm == 3 and carrier.startswith("comb"):
        # a second task on a leaf of joint 1: two constraint blocks in different subtrees
        wl = helpers.multi_task_batch(model, B, [link, 2], seed, nu_scale=0.3)
    else:
        wl = helpers.feasible_batch(model, B, link, seed, nu_scale=0.3)
    if not plain:
        wl["H_ref"], wl["v_ref"] = reference_weight(hm), V_REF
    wl["refs"] = None
    if hm == 3:
        from test_formulation_editing import per_link_references
        wl["refs"] = per_link_references(model, 5)
    wl["model"], wl["num_eq_c"] = model, len(wl["c_ids"])
    for v in wl.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)      # shared among the tests that need it: left unchanged
    return wl


def workload(rc):
    return _workload(rc.carrier, batch_of(rc), rc.hm, False, seed_of(rc.carrier, batch_of(rc), rc.hm, rc.mur == 1))


def plain_workload(carrier):
    """the default launch of the edge-shape test: H_ref = I, v_ref = 0 as the generator leaves them, B = 130"""
    return _workload(carrier, 130, 0, True, DEFAULT_SEED)


def solve_args(wl, b=None):
    if b is None:
        return (wl["q"], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"], wl["lb"], wl["ub"])
    return (wl["q"][b], wl["H_ref"], wl["v_ref"], wl["c_ids"], wl["Ais"], wl["bis"][b], wl["lb"], wl["ub"])


def params(wl, osqp, **kw):
    return dict(FIXTURE, num_eq_c=wl["num_eq_c"], mu_update_strat=1 if osqp else 0, **kw)


END_TO_END = dict(max_iter=400, tol_abs=1e-6, tol_rel=0.0)
_ORACLE = {}


def oracle_end_to_end(wl, osqp):
    """ref.solve_batch of the workload under the end-to-end parameters, once per (workload, rule)"""
    key = (id(wl), bool(osqp))
    if key not in _ORACLE:
        _ORACLE[key] = ref.solve_batch(wl["model"], *solve_args(wl), nthreads=8, want_nu=True, refs=wl["refs"], **params(wl, osqp, **END_TO_END))
    return _ORACLE[key]


# ---- k iterations, field by field: the instances compared, and how well the comparison is posed there ----------------------------
K_ITERATIONS = (2, 7)       # (with a slice of 5, seven iterations cross a slice boundary)
SAMPLE_EVERY = 37
FIELD_NAMES = ["nu", "z", "w", "vis", "fis", "g", "yis", "Aty", "Stf_plus_w", "primal_residual_vec", "dual_residual_vec"]   # (test_engines.FIELDS)


def k_params(wl, osqp, k):
    return params(wl, osqp, max_iter=k + 1, tol_abs=0.0, tol_rel=1e-30, tol_primal_inf=0.0)


def solve(s, wl, b=None, args=None):
    """the device handle or the oracle's solver: per-link weights go in through SolveInit, UpdateReferences, Solve()"""
    args = solve_args(wl, b) if args is None else args
    if wl["refs"] is None:
        s.Solve(*args)
    else:
        s.SolveInit(*args); s.UpdateReferences(*wl["refs"]); s.Solve()


def distance(a, b):
    """the abs-or-rel distance helpers.assert_close bounds"""
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    if a.size == 0:
        return 0.0
    d = np.abs(a - b)
    return float(np.minimum(d, d / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)).max())


def oracle_sensitivity(wl, osqp, k, b, scalars, n_perturbations=6, eps=1e-15):
    """How far the ORACLE's own fields after k iterations move when q and b of instance `b` are perturbed by a relative 1e-15 -- a few
    roundings' worth: the largest abs-or-rel distance over the compared fields and `n_perturbations` draws.  Where this is large the
    comparison is ill posed whoever computes: the rule that moves mu compares residuals (decade steps: primal > 10 dual) or divides them
    (OSQP's), and once both are rounding errors -- a star's instance is there after six iterations -- or sit on the threshold, one
    rounding decides.  No device involved."""
    def run(args):
        r = ref.RefSolver(wl["model"], **k_params(wl, osqp, k))
        solve(r, wl, args=args)
        return [r.field(n) for n in FIELD_NAMES] + [r.His[1:]] + [r.scalar(n) for n in scalars]
    base = run(solve_args(wl, b))
    rng = np.random.default_rng(1000 * k + b)
    worst = 0.0
    for _ in range(n_perturbations):
        a = list(solve_args(wl, b))
        a[0] = a[0] * (1.0 + eps * rng.uniform(-1, 1, a[0].shape))
        a[5] = a[5] * (1.0 + eps * rng.uniform(-1, 1, a[5].shape))
        worst = max(worst, max(distance(x, y) for x, y in zip(base, run(a))))
    return worst


def plan_kernel(plan):
    """the iteration kernel a handle's plan names, and its "N ancestors per joint\""""
    m = re.search(r"k_fslots \+ (k_flat2|k_flat1|k_flat)[ (]", plan)
    n = re.search(r"(\d+) ancestors per joint", plan)
    return (m.group(1) if m else None), (int(n.group(1)) if n else None)
