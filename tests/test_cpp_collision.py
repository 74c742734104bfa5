"""The collision calls through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_collision.h) compile and link
(CPU); tests/cpp/test_collision.cpp runs on the GPU, and what its two Clearance calls return is what the Python binding returns, bit for
bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_collision_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_collision.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_collision")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_collision_runs_and_matches_the_binding(tmp_path):
    import loik_amd
    from test_pose_ik import _handle
    test_cpp_collision_compiles()
    dump = str(tmp_path / "collision.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_collision"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all collision checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    # the same calls through the binding, on the same configurations and the same model (sixteenths and sixty-fourths: the same doubles
    # in both languages)
    model = loik_amd.builtin_model("panda7")
    B = 67
    q0 = np.array([[((b * 7 + 3 * k) % 17 - 8) / 16.0 for k in range(model.nq)] for b in range(B)])
    links, spheres = [], []
    for l in range(1, 8):
        for k in range(2):
            links.append(l)
            spheres.append([((l + k) % 5 - 2) / 64.0, ((2 * l + k) % 7 - 3) / 64.0, (4 if k else -3) / 64.0, (2 + (l + k) % 3) / 64.0])
    s, _ = _handle(model, B, [7], q0)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world([[0.25, 0.0, 0.5, 0.125], [-0.5, 0.25, 0.25, 0.0625]], [(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -0.25], [0, 0, 0, 1.0]]), [1.0, 1.0, 0.125])])
    s.set_self_collision(True, ignore=[(2, 4)])
    assert s.num_self_pairs() == 56
    want = []
    for r in (s.clearance(), s.clearance(q0[3:8])):
        want += [r["min"], r["min_world"], r["min_self"], r["witness"].astype(np.float64).ravel()]
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
