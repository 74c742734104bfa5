"""CPU: the numpy reference of the shortcut rule (tests/shortcut_numpy.py) keeps what include/loik_amd_shortcut.h promises: the segments it
accepts are free on dense samples, every draw is a proper sub-path, the ends stay, and no rounds is the identity."""
import numpy as np

import motion_numpy as MN
import pose_multistart_numpy as MS
import shortcut_numpy as SN
import test_shortcut as TS


def test_accepted_segments_are_free_on_dense_samples():
    c = TS.shortcut_case("panda7")
    model, paths, want = c["model"], c["paths"], c["want"]
    ss = np.linspace(0.0, 1.0, 200)
    seen = 0
    for b in range(c["B"]):
        for i, j, st in want["segments"][b]:
            if st != MN.FREE:
                continue
            seen += 1
            dv = MN.difference(model, paths[b, i], paths[b, j])[0]
            q = MN.interpolate_many(model, paths[b, i], dv, ss)
            assert np.allclose(q[-1], paths[b, j], rtol=0, atol=1e-12)
            clear = MN.clearance_min(model, q, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"])
            assert np.all(clear >= c["margin"]), (b, i, j, clear.min(), c["margin"])
    assert seen == want["accepted"].sum() > 0


def test_every_draw_is_a_proper_sub_path():
    for L in list(range(3, 40)) + [64, 65, 1000, 2 ** 31 - 1]:
        for r in range(6):
            for b in (0, 1, 77, 2 ** 31 - 1):
                i, j = SN.draw(4242 + L, r, b, L)
                assert 0 <= i < j - 1 <= L - 2, (L, r, b, i, j)
    # every admissible pair of a short path turns up, and the draw is the sampler's word
    w = MS.words(1, 9, 3, np.arange(2))
    assert SN.draw(1, 9, 3, 5) == (int(w[0] % np.uint64(3)), int(w[0] % np.uint64(3)) + 2 + int(w[1] % np.uint64(3 - int(w[0] % np.uint64(3)))))
    seen = {SN.draw(1, r, 0, 5) for r in range(400)}
    assert seen == {(i, j) for i in range(3) for j in range(i + 2, 5)}


def test_the_ends_stay_and_keep_increases():
    for name in ("panda7", "multidof13"):
        c = TS.shortcut_case(name)
        want, T = c["want"], c["paths"].shape[1]
        for b in range(c["B"]):
            L, keep = int(want["n_waypoints"][b]), want["keep"][b]
            assert 2 <= L <= T and keep[0] == 0 and keep[L - 1] == T - 1 and np.all(np.diff(keep[:L]) > 0) and np.all(keep[L:] == -1)
            assert np.array_equal(want["q_path"][b, :L], c["paths"][b, keep[:L]]) and np.all(want["q_path"][b, L:] == c["paths"][b, T - 1])
            assert want["tried"][b] == want["accepted"][b] + want["blocked"][b] + want["undecided"][b] + want["invalid"][b]
            assert L == 2 or want["tried"][b] == TS.ROUNDS
        assert (want["n_waypoints"] == 2).any() and (want["n_waypoints"] == T).any()


def test_no_rounds_is_the_identity():
    c = TS.shortcut_case("panda7")
    paths = c["paths"]
    B, T = paths.shape[:2]
    got = SN.shortcut(c["model"], paths, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], **dict(c["kw"], rounds=0))
    assert np.array_equal(got["q_path"], paths) and np.all(got["keep"] == np.arange(T)) and np.all(got["n_waypoints"] == T)
    assert all(np.all(got[k] == 0) for k in TS.COUNTERS[1:]) and np.array_equal(got["length_in"], got["length_out"])
    assert np.array_equal(got["length_in"], SN.path_length(c["model"], paths)) and np.all(got["length_in"] > 0.0)
    # a skipped path, and counts of 0 and 1 for the length
    n = np.array([0, 1, 2, T, T + 1] + [T] * (B - 5))
    got = SN.shortcut(c["model"], paths, c["links"], c["spheres"], c["ws"], c["wb"], c["pairs"], n_waypoints=n, **c["kw"])
    for b in (0, 1, 4):
        assert np.all(got["keep"][b] == -1) and np.isnan(got["q_path"][b]).all() and all(got[k][b] == 0 for k in TS.COUNTERS) and np.isnan(got["length_in"][b])
    assert got["n_waypoints"][2] == 2 and got["tried"][2] == 0
    ln = SN.path_length(c["model"], paths, n)
    assert ln[0] == 0.0 and ln[1] == 0.0 and ln[2] > 0.0 and np.isnan(ln[4])
