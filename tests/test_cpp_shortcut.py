"""The shortcut calls through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_shortcut.h) compile and link (CPU);
tests/cpp/test_shortcut.cpp runs on the GPU, and what its ShortcutPaths and PathLength calls return is what the Python binding returns,
bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_motion import cpp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_shortcut_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_shortcut.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_shortcut")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_shortcut_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_shortcut_compiles()
    dump = str(tmp_path / "shortcut.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_shortcut"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all shortcut checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, dv, links, spheres, ws, box = cpp_case()
    B, T = qa.shape[0], 4
    paths = np.ascontiguousarray(qa[:B // T * T].reshape(B // T, T, model.nq))
    s, _ = _handle(model, B, [7], qa)
    want = [s.path_length(paths)]
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, [box])
    s.set_self_collision(True, ignore=[(2, 4)])
    kw = dict(rounds=6, seed=99, margin=-0.0625, tol=1.0 / 1024, max_evals=64)
    n = np.arange(B // T, dtype=np.int32) % (T + 2)
    for r in (s.shortcut_paths(paths, **kw), s.shortcut_paths(paths, n_waypoints=n, **kw)):
        want += [r[k].astype(np.float64).ravel() for k in ("q_path", "n_waypoints", "keep", "tried", "accepted", "blocked", "undecided", "invalid",
                                                         "length_in", "length_out")]
    want.append(s.path_length(paths, n_waypoints=n))
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
