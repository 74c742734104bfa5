"""The avoidance calls through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_avoid.h) compile and link (CPU);
tests/cpp/test_avoid.cpp runs on the GPU, and what its ClearanceGradient, AvoidanceBox and latched SolvePose return is what the Python
binding returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_motion import cpp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_avoid_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_avoid.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_avoid")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_avoid_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_avoid_compiles()
    dump = str(tmp_path / "avoid.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_avoid"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all avoidance checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, _, links, spheres, ws, box = cpp_case()
    s, _ = _handle(model, qa.shape[0], [7], qa)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, [box])
    s.set_self_collision(True, ignore=[(2, 4)])
    prm = dict(d_safe=1.0 / 64, d_influence=0.25, kappa=0.5)
    g = s.clearance_gradient()
    b = s.avoidance_box(qa, 0.25, -2.0, 2.0, **prm)
    s.set_collision_avoidance(**prm)
    target = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.375, 0.125, 0.5])
    r = s.SolvePose(target, dt=0.25, gain=0.5, tol_pose=1e-4, max_steps=2, q=qa)
    s.close()
    want = np.concatenate([a.astype(np.float64).ravel() for a in (g["grad"], g["min"], g["witness"], b["lo"], b["hi"], b["pairs"], b["partner"],
                                                                  r["avoid_min_seen"], r["avoid_active_steps"], r["avoid_flags"])])
    assert got.shape == want.shape and np.array_equal(got, want)
