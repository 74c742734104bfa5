"""The voxel world through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_grid.h) compiles and links (CPU);
tests/cpp/test_grid.cpp runs on the GPU, and the field, the clearances and the motion checks it dumps are what the Python binding returns,
bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_motion import cpp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_grid_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_grid.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_grid")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_grid_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_grid_compiles()
    dump = str(tmp_path / "grid.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_grid"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all grid checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, dv, links, spheres, ws, box = cpp_case()
    s, _ = _handle(model, qa.shape[0], [7], qa)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, [box])
    s.set_self_collision(True, ignore=[(2, 4)])
    z, y, x = np.meshgrid(np.arange(7), np.arange(8), np.arange(9), indexing="ij")
    s.set_collision_grid((x * 7 + y * 5 + z * 3) % 23 == 0, (-0.5, -0.5, 0.0), 0.125)
    clr = s.clearance()
    mot = s.motion_clearance(qa, dv=dv, margin=-0.0625, tol=1.0 / 1024, max_evals=16)
    want = [s.collision_grid()["G"].astype(np.float64).ravel()]
    want += [clr[k].astype(np.float64).ravel() for k in ("min", "min_world", "min_self", "witness")]
    want += [mot[k].astype(np.float64).ravel() for k in ("status", "evals", "s_free", "min_sampled", "s_at_min", "witness")]
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
