"""The motion calls through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_motion.h) compile and link (CPU);
tests/cpp/test_motion.cpp runs on the GPU, and what its Difference, MotionClearance and PathClearance calls return is what the Python
binding returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_motion_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_motion.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_motion")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def cpp_case():
    """the model, configurations, displacements and spheres of tests/cpp/test_motion.cpp: the same doubles in both languages"""
    import loik_amd
    model = loik_amd.builtin_model("panda7")
    B = 67
    qa = np.array([[((b * 7 + 3 * k) % 17 - 8) / 16.0 for k in range(model.nq)] for b in range(B)])
    dv = np.array([[((b * 5 + 11 * k) % 23 - 11) / 64.0 for k in range(model.nv)] for b in range(B)])
    links, spheres = [], []
    for l in range(1, 8):
        for k in range(2):
            links.append(l)
            spheres.append([((l + k) % 5 - 2) / 64.0, ((2 * l + k) % 7 - 3) / 64.0, (4 if k else -3) / 64.0, (2 + (l + k) % 3) / 64.0])
    ws = [[0.25, 0.0, 0.5, 0.125], [-0.5, 0.25, 0.25, 0.0625]]
    box = (np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -0.25], [0, 0, 0, 1.0]]), [1.0, 1.0, 0.125])
    return model, qa, dv, links, spheres, ws, box


@pytest.mark.gpu
def test_cpp_motion_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_motion_compiles()
    dump = str(tmp_path / "motion.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_motion"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all motion checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, dv, links, spheres, ws, box = cpp_case()
    B, T = qa.shape[0], 4
    s, _ = _handle(model, B, [7], qa)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, [box])
    s.set_self_collision(True, ignore=[(2, 4)])
    margin, tol = -0.0625, 1.0 / 1024
    want = [s.difference(qa, qa + dv).ravel()]
    path = s.path_clearance(qa[:B // T * T].reshape(B // T, T, model.nq), margin=margin, tol=tol, max_evals=16)
    for r in (s.motion_clearance(qa, dv=dv, margin=margin, tol=tol, max_evals=16), s.motion_clearance(qa, dv=dv, margin=margin, tol=tol, max_evals=1),
              {k: v.reshape((-1,) + v.shape[2:]) for k, v in path.items()}):
        want += [r[k].astype(np.float64).ravel() for k in ("status", "evals", "s_free", "min_sampled", "s_at_min", "witness")]
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
