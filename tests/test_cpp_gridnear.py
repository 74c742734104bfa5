"""The nearest-voxel transform through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_gridnear.h) compiles
and links (CPU); tests/cpp/test_gridnear.cpp runs on the GPU, and the transform, the query, the gradient and the box it dumps are what
the Python binding returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_motion import cpp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_gridnear_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_gridnear.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_gridnear")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_gridnear_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_gridnear_compiles()
    dump = str(tmp_path / "gridnear.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_gridnear"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all gridnear checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, dv, links, spheres, ws, box = cpp_case()
    s, _ = _handle(model, qa.shape[0], [7], qa)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, [box])
    s.set_self_collision(True, ignore=[(2, 4)])
    z, y, x = np.meshgrid(np.arange(7), np.arange(8), np.arange(9), indexing="ij")
    s.set_collision_grid((x * 7 + y * 5 + z * 3) % 23 == 0, (-0.5, -0.5, 0.0), 0.125)
    s.set_collision_grid_nearest(True)
    i = np.arange(40)
    qs = np.stack([((i * 7) % 19 - 9) / 16.0 + 1.0 / 256, ((i * 5) % 17 - 8) / 16.0 + 1.0 / 512, ((i * 3) % 13) / 16.0 + 3.0 / 1024, (i % 4) / 64.0], axis=1)
    nr = s.grid_nearest(qs)
    grad = s.clearance_gradient()
    bx = s.avoidance_box(None, 0.25, -2.0, 2.0, 0.015625, 0.125, 0.5)
    want = [s.collision_grid_nearest().astype(np.float64).ravel()]
    want += [nr[k].astype(np.float64).ravel() for k in ("val", "vox", "normal")]
    want += [grad["grad"].ravel()] + [bx[k].astype(np.float64).ravel() for k in ("lo", "hi", "pairs", "partner")]
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
