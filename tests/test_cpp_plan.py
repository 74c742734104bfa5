"""The planning call through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_plan.h) compiles and links (CPU);
tests/cpp/test_plan.cpp runs on the GPU, and what its PlanPaths calls return is what the Python binding returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_motion import cpp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_plan_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_plan.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_plan")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_plan_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_plan_compiles()
    dump = str(tmp_path / "plan.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_plan"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all plan checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, dv, links, spheres, ws, box = cpp_case()
    B, Bq, T = qa.shape[0], 16, 16
    s, _ = _handle(model, B, [7], qa)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, [box])
    s.set_self_collision(True, ignore=[(2, 4)])
    kw = dict(step=0.5, max_nodes=32, seed=99, margin=-0.0625, tol=1.0 / 1024, max_evals=64)
    want = []
    for iters in (16, 0):
        r = s.plan_paths(qa[:Bq], qa[Bq:2 * Bq], -1.0, 1.0, T, max_iters=iters, **kw)
        want += [r[k].astype(np.float64).ravel() for k in ("q_path", "n_waypoints", "status", "iterations", "nodes", "edges_checked", "edges_free",
                                                         "evals", "length")]
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
