"""The inputs of tests/test_avoid_big.py, built without a GPU and computed once: the step mode of k_avoid_box (loik_pose_avoid.hpp) on
the 170- and the 330-joint tree of test_clearance.py, whose DoFs stride past one wavefront, with sphere counts on either side of the
64 KB rule that sends the placements to HBM.  One task on the deepest leaf (root paths of 66 and 154 joints), a sphere per link, cut
to `ns` of them (sphere_links says which, and why).

With make_spheres' stock radii and test_clearance._world every instance of these trees starts in penetration: r = 0, every bound is 0,
and a test says little.  So the radii are scaled by RADIUS_SCALE, and of the world objects drawn only those are kept that leave every
sphere of every seed more than d_safe + WORLD_MARGIN (thinned_world).  tests/test_avoid_big_numpy.py asserts on the reference alone
what makes each case a test."""
import numpy as np

from test_pose_ik import BOUND
from test_pose_parity import _box, _nonsym_A, _seeds
from test_avoid_pose import AVOID, LAWS
import clearance_numpy as CN
import pose_accel_numpy as PA
import pose_limits_numpy as PL
import pose_numpy as P
import test_avoid_routes as R
import test_clearance as TC

RADIUS_SCALE = 0.25
WORLD_MARGIN = 0.01
WORLD_DRAWN = (24, 20)   # world spheres and boxes drawn; at most (6, 5) of those that pass are kept
WORLD_KEPT = (6, 5)
SPREAD = (1e-3, 0.3)
LAW = LAWS[0]            # (0.25, 0.5)
STEPS = (1, 2)
CLR_WAVES, LDS_BYTES, AVD_ENTRY = 4, 65536, 5
_WORK, _MODELS = {}, {}


# ---- the launch shape, from the formula of loik_pose_avoid.hpp and the rule of loik_host_pose.hpp ------------------------------------------
def wave_doubles(nb, ns, hbm):
    """avd_wave_doubles: centres [ns][4], tv [ns][2], list [2 ns][AVD_ENTRY], then (ints) to [ns][2], sj [ns], anc [nb][W]; without HBM
    placements liM [nb][12] and oMi [nb][12] as well"""
    W = (nb + 31) >> 5
    return (4 + 2 + 2 * AVD_ENTRY + 1) * ns + (ns + 1) // 2 + (nb * W + 1) // 2 + (0 if hbm else 24 * nb)


def launch_shape(nb, ns):
    """(HBM placements, wavefronts per workgroup) of avoid_launch: HBM when one wavefront's LDS stages do not fit 64 KB; then the largest
    power of two of wavefronts, CLR_WAVES at most, that fits (lds_waves)"""
    hbm = wave_doubles(nb, ns, False) * 8 > LDS_BYTES
    per = wave_doubles(nb, ns, hbm) * 8
    waves = CLR_WAVES
    while waves > 1 and waves * per > LDS_BYTES:
        waves >>= 1
    return hbm, waves


# (robot, ns, HBM, wavefronts per workgroup, B, seed): B = 3 at two wavefronts leaves a ragged last workgroup.  The seeds are the first
# from x000 on for which test_avoid_big_numpy.test_table_inputs holds
TABLE = [
    ("tree170", 64, False, 1, 5, 3000),
    ("tree170", 205, False, 1, 5, 3100),
    ("tree170", 206, True, 1, 5, 3100),
    ("tree330", 100, True, 2, 3, 3301),
    ("tree330", 256, True, 1, 3, 3401),
]


def row_id(c):
    return "%s-ns%d-%s" % (c[0], c[1], "hbm" if c[2] else "lds")


def row(name, ns):
    return next(c for c in TABLE if c[:2] == (name, ns))


# ---- the workloads --------------------------------------------------------------------------------------------------------------------------
def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = TC._model(name)
    return _MODELS[name]


def deepest_leaf(model):
    """(the joint with the longest root path, the lowest index on a tie; the number of joints on that path)"""
    depth = np.zeros(model.njoints, dtype=int)
    for i in range(1, model.njoints):
        depth[i] = depth[int(model.parents[i])] + 1
    return int(np.argmax(depth)), int(depth.max())


def sphere_links(model, ns):
    """a sphere per link, dealt from the LAST link down (and round again where ns exceeds the links: 205 and 206 on tree170), cut to ns.
    From the leaf end, not the root end: H_ref weighs the spatial velocity of every link, so the z of a step falls by a decade every few
    joints from the task's leaf toward the root (1e-2 at the leaf, 1e-7 forty joints up), and spheres on the first links would narrow
    only DoFs whose z is far inside any bound -- no entry would ever rest on one"""
    nb = model.njoints - 1
    return [nb - s % nb for s in range(ns)]


def thinned_world(model, q0, links, spheres, rng):
    """test_clearance._world(rng, *WORLD_DRAWN), of which the first WORLD_KEPT objects are kept that leave every sphere at every seed a
    clearance above d_safe + WORLD_MARGIN"""
    ws, wb = TC._world(rng, *WORLD_DRAWN)
    cen = CN.centres(model, q0, links, spheres)
    floor = AVOID["d_safe"] + WORLD_MARGIN
    ks = [o for o in range(ws.shape[0]) if np.min(CN.sphere_sphere(cen, spheres[None, :, 3], ws[o, :3], ws[o, 3])) > floor][:WORLD_KEPT[0]]
    kb = [o for o in range(wb.shape[0]) if np.min(CN.sphere_box(cen, spheres[None, :, 3], wb[o])) > floor][:WORLD_KEPT[1]]
    return ws[ks], wb[kb]


def workload(name, ns, variant=0, box_inst=False, a_inst=False, B=5, seed=0, f32_box=False):
    """test_avoid_routes.route_workload on a big tree: variant 0 no limits, 1 binding position limits, 2 position and acceleration limits;
    the base box shared (BOUND) or per instance; A shared or per instance.  q_t [B][nq]: the configurations the targets were drawn from"""
    key = (name, ns, variant, box_inst, a_inst, B, seed, f32_box)
    if key in _WORK:
        return _WORK[key]
    model = model_of(name)
    links = [deepest_leaf(model)[0]]
    rng = np.random.default_rng(seed)
    A = _nonsym_A(rng, 1, B if a_inst else None)
    q0, tg = _seeds(model, B, links, seed=seed + 1, spread=SPREAD)
    q_t = model.random_configurations(np.random.default_rng(seed + 1), B)   # (what _seeds drew the targets from)
    q_lo, q_hi = -np.inf * np.ones(model.nv), np.inf * np.ones(model.nv)
    a_max = None
    if variant >= 1:
        q_lo, q_hi, q0 = PL.binding_limits(model, q_t, q0, seed + 2, (10.0, 90.0))
    if variant == 2:
        a_max = PA.accel_limits(model, seed + 3, LAW[0], BOUND, lo=0.05, hi=0.5)
    lk, spheres = CN.make_spheres(model, 1, seed + 4, links=sphere_links(model, ns))
    spheres[:, 3] *= RADIUS_SCALE
    ws, wb = thinned_world(model, q0, lk, spheres, rng)
    col = dict(links=lk, spheres=spheres, ws=ws, wb=wb, pairs=CN.self_pairs(model.parents, lk))
    box = R._inst_box(rng, B, model.nv, f32_box) if box_inst else _box(model)
    _WORK[key] = dict(model=model, links=links, A=A, q0=q0, q_t=q_t, tg=tg, q_lo=q_lo, q_hi=q_hi, a_max=a_max, box=box, B=B, col=col, ns=ns, name=name)
    return _WORK[key]


def table_case(c, box_inst=False):
    """the containment workload of a row of TABLE: no limits, the box on the fp32 grid"""
    return workload(c[0], c[1], 0, box_inst, False, c[4], c[5], f32_box=True)


# lock-step parity: (what, robot, ns, variant, per-instance box, per-instance A, seed), B = 5.  One case per route without limits on the
# shared box, an HBM case through the tiles (binding position and acceleration limits) and an HBM case over the per-instance box and A
PARITY = [
    ("lds-nolimits", "tree170", 64, 0, False, False, 3500),
    ("hbm-nolimits", "tree330", 100, 0, False, False, 3600),
    ("hbm-limits-accel", "tree170", 206, 2, False, False, 3702),
    ("hbm-boxinst-Ainst", "tree330", 100, 0, True, True, 3800),
]
PARITY_B = 5


def parity_case(c):
    return workload(c[1], c[2], c[3], c[4], c[5], PARITY_B, c[6])


# the base box comes back, and the loops beside SolvePose
BACK = ("tree170", 206, 3900)
LOOPS = ("tree330", 100, 4000)
TRACK_T = 2


def back_case():
    return workload(BACK[0], BACK[1], 0, True, False, 5, BACK[2])


def loops_case():
    return workload(LOOPS[0], LOOPS[1], 0, False, False, 5, LOOPS[2])


def track_samples(w, T=TRACK_T):
    """[B][T + 1][1][12]: the task frame along the straight joint-space line from each seed to the configuration its target was drawn
    from (these trees have nq == nv: a plain difference)"""
    model, B = w["model"], w["B"]
    assert model.nq == model.nv
    qs = np.stack([[w["q0"][b] + (k / T) * (w["q_t"][b] - w["q0"][b]) for k in range(T + 1)] for b in range(B)])
    return P.fk12(model, qs.reshape(-1, model.nq), w["links"]).reshape(B, T + 1, len(w["links"]), 12)


# ---- what the CPU file asserts ------------------------------------------------------------------------------------------------------------
def start_clearance(w):
    """the least clearance of every seed [B]"""
    c = w["col"]
    return CN.clearance(w["model"], w["q0"], c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])["min"]


def resting_dofs(w, law):
    """the DoF indices of the entries test_avoid_routes.resting_on_narrowed counts"""
    return np.flatnonzero(R.resting_entries(w, law).any(axis=0))
