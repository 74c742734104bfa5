"""The flat engine's static schedule of a kinematic tree (loikb_flat_schedule; loik_amd/csrc/loik_flat.hpp): the host-side
tables that let k_flat replace the level-by-level recursions of LoikBackwardStepVisitor / LoikForwardStep2Visitor
(/root/reference/include/loik/loik-loid-optimized.hxx:31-81, :102-163) by sums over subtrees and root paths.  Emulated here
lane by lane in numpy, the way the kernel uses them, against the sums written out directly.  No GPU needed."""
import numpy as np
import pytest

import loik_amd
from loik_amd import capi
from helpers import caterpillar_parents, comb_parents, random_tree, star_parents


def _tree(parents):
    parents = np.asarray(parents)
    nj = parents.size
    depth = np.zeros(nj, int)
    for i in range(1, nj):
        depth[i] = 1 if parents[i] == 0 else depth[parents[i]] + 1
    anc = [[] for _ in range(nj)]   # strict ancestors, nearest first
    for i in range(1, nj):
        a = parents[i]
        while a > 0:
            anc[i].append(a)
            a = parents[a]
    desc = [[d for d in range(1, nj) if i in anc[d]] for i in range(nj)]
    return depth, anc, desc


def _models():
    out = [(n, loik_amd.builtin_model(n).parents) for n in ("talos32", "talos44")]
    for seed, nb, bp in [(3, 21, 0.35), (8, 30, 0.35), (11, 40, 0.35), (3, 60, 0.6), (5, 60, 0.6)]:
        out.append(("tree%d_%d" % (seed, nb), random_tree(seed, nb, branch_prob=bp).parents))
    # the carriers of the flat kernels' census (tests/flat_census.py): the limits of depth and lane count, by construction
    for nb, depth in [(32, 11), (32, 12), (17, 17), (33, 11), (33, 12), (64, 17)]:
        out.append(("comb%d_%d" % (nb, depth), np.array(comb_parents(nb, depth))))
    for nb, depth in [(24, 17), (33, 17)]:
        out.append(("caterpillar%d_%d" % (nb, depth), np.array(caterpillar_parents(nb, depth))))
    for nb in (17, 33):
        out.append(("star%d" % nb, np.array(star_parents(nb))))
    return out


@pytest.mark.parametrize("name,parents", _models())
def test_tables_describe_the_tree(name, parents):
    fs = capi.flat_schedule(parents)
    assert fs is not None, (name, capi.lib().loikb_last_error())
    depth, anc, desc = _tree(parents)
    nb = len(parents) - 1
    G = fs["G"]
    assert G >= nb and G in (8, 16, 32, 64) and (G == 8 or G // 2 < nb)
    assert fs["nanc"] == max(1, depth.max() - 1) and (1 << fs["njmp"]) >= depth.max() and (1 << fs["nscan"]) > max(len(d) + 1 for d in desc[1:])
    for l in range(nb):
        i = l + 1
        assert fs["depth"][l] == depth[i] and fs["size"][l] == len(desc[i]) + 1
        # depth-first numbering: the subtree is the contiguous range of lanes behind the joint
        assert sorted(desc[i]) == list(range(i + 1, i + 1 + len(desc[i])))
        for r in range(5):
            want = anc[i][(1 << r) - 1] - 1 if len(anc[i]) >= (1 << r) else -1
            assert fs["jmp"][l, r] == want, (name, l, r)
        for k in range(16):
            want = [a for a in anc[i] if depth[a] == k + 1]
            assert fs["anc"][l, k] == (want[0] - 1 if want else -1)
    assert np.all(fs["depth"][nb:] == 0) and np.all(fs["size"][nb:] == 0)


@pytest.mark.parametrize("name,parents", _models())
def test_subtree_sums_by_window_doubling(name, parents):
    """flat_subtree_sum / the scan inside k_flat: B_k[i] = x_i + ... + x_{i + 2^k - 1} by doubling, every lane adds the windows
    that tile [i, i + size_i), low bits of size first, the last two bits in one exchange; only members of the subtree are added"""
    fs = capi.flat_schedule(parents)
    _, _, desc = _tree(parents)
    nb, G, nscan = len(parents) - 1, fs["G"], fs["nscan"]
    rng = np.random.default_rng(1)
    x = np.zeros(G + 1)          # (row G: the zero row)
    x[:nb] = rng.uniform(0.5, 1.5, nb)   # positive: a sum over anything but the subtree's members would show
    size = fs["size"]
    B = x[:G].copy(); S = np.zeros(G); pos = np.arange(G)

    def row(r, rows):
        return np.where(r < G, rows[np.minimum(r, G - 1)], 0.0)

    kk = 0
    while kk + 2 < nscan or (kk < 2 and kk < nscan):   # plain steps (the kernel always runs steps 0 and 1)
        rows = B.copy()
        take = (size >> kk) & 1
        S += np.where(take == 1, row(pos, rows), 0.0)
        B = rows + row(np.arange(G) + (1 << kk), rows)
        pos = pos + take * (1 << kk)
        kk += 1
    if kk < nscan:   # the last two bits in one exchange
        rows = B.copy()
        w = 1 << kk
        t0, t1 = (size >> kk) & 1, (size >> (kk + 1)) & 1
        p1 = pos + t0 * w
        S += np.where(t0 == 1, row(pos, rows), 0.0) + np.where(t1 == 1, row(p1, rows) + row(p1 + w, rows), 0.0)
    want = np.array([x[l] + sum(x[d - 1] for d in desc[l + 1]) for l in range(nb)])
    assert np.allclose(S[:nb], want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("name,parents", _models())
def test_path_sums_by_pointer_jumping(name, parents):
    fs = capi.flat_schedule(parents)
    _, anc, _ = _tree(parents)
    nb, G = len(parents) - 1, fs["G"]
    rng = np.random.default_rng(2)
    y = np.zeros(G + 1)
    y[:nb] = rng.uniform(0.5, 1.5, nb)
    for r in range(fs["njmp"]):
        rows = y.copy()
        j = fs["jmp"][:, r]
        y[:G] = rows[:G] + np.where(j >= 0, rows[np.maximum(j, 0)], 0.0)
    x0 = np.zeros(G); x0[:nb] = np.random.default_rng(2).uniform(0.5, 1.5, nb)
    want = np.array([x0[l] + sum(x0[a - 1] for a in anc[l + 1]) for l in range(nb)])
    assert np.allclose(y[:nb], want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("name,parents", _models())
def test_rows_of_w_tau_are_dealt_out_completely(name, parents):
    """r'_a = tau_a + sum_{d below a} W_{a,d} tau_d: lane a sums up to 8 of its row's products (entry (depth_a - 1) * G + lane
    of d), the rest goes in chunks of 8 to lanes without a row of their own, which publish partial sums; every product
    is summed exactly once, by the right joint"""
    fs = capi.flat_schedule(parents)
    depth, _, desc = _tree(parents)
    nb, G = len(parents) - 1, fs["G"]
    prod = np.random.default_rng(3).uniform(0.5, 1.5, (16, G))   # prod[k, lane d] = W_{anc_k(d), d} tau_d
    acc = np.zeros(G)
    for l in range(G):
        for e in fs["red"][l]:
            if e >= 0:
                acc[l] += prod[e // G, e % G]
    helper = fs["helper"].astype(bool)
    own = np.where(helper, 0.0, acc)
    for l in range(G):
        for h in fs["part"][l]:
            if h >= 0:
                assert helper[h], "a partial comes from a helper lane"
                own[l] += acc[h]
    used = [e for l in range(G) for e in fs["red"][l] if e >= 0]
    assert len(used) == len(set(used)) == sum(len(d) for d in desc[1:]), "every (ancestor, joint) product exactly once"
    for l in range(nb):
        want = sum(prod[depth[l + 1] - 1, d - 1] for d in desc[l + 1])
        assert np.isclose(own[l], want, rtol=1e-14, atol=0), (name, l)
    # helpers have no row of their own, and are each used once
    hs = [h for l in range(G) for h in fs["part"][l] if h >= 0]
    assert len(hs) == len(set(hs)) == int(helper.sum())
    for h in hs:
        assert h >= nb or len(desc[h + 1]) == 0


def test_where_the_engine_does_not_apply():
    # joints not numbered depth-first: subtrees are not contiguous ranges
    assert capi.flat_schedule([0, 0, 0, 1, 2, 3, 4]) is None
    assert b"depth-first" in capi.lib().loikb_last_error()
    # a chain deeper than the ancestor table
    assert capi.flat_schedule([0] + list(range(0, 30))) is None
    # a deep 60-joint tree in 64 lanes: its long rows would need more helper lanes than there are leaves
    assert capi.flat_schedule(random_tree(11, 60).parents) is None
    assert b"too many descendants" in capi.lib().loikb_last_error()
    # more joints than lanes
    assert capi.flat_schedule([0] + [0] * 70) is None
    # a star: every joint a child of the universe -- trivially fine
    fs = capi.flat_schedule([0] + [0] * 20)
    assert fs is not None and fs["nanc"] == 1 and np.all(fs["size"][:20] == 1)
