"""Depth images and point clouds through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_depth.h) compile and
link (CPU); tests/cpp/test_depth.cpp runs on the GPU, and the counters, occupancies, fields and clearances it dumps are what the Python
binding returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_motion import cpp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_depth_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_depth.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_depth")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_depth_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_depth_compiles()
    dump = str(tmp_path / "depth.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_depth"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all depth checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, dv, links, spheres, ws, box = cpp_case()
    s, _ = _handle(model, qa.shape[0], [7], qa)
    s.set_collision_spheres(links, spheres)
    cam = dict(fx=32.0, fy=32.0, cx=19.5, cy=14.5, T_world_cam=[0, 0, 1, -1, 0, 0, 0, -1, 0, -1.0, 0.0, 0.375], z_min=0.25, z_max=8.0)
    dims, origin, voxel = (19, 17, 15), np.array([-0.5, -0.53125, -0.03125]) + 1.0 / 8192, 0.0625
    v, u = np.meshgrid(np.arange(30), np.arange(40), indexing="ij")
    f1 = np.where((u * 7 + v * 5) % 29 == 0, 0.0, 0.625 + ((u * 7 + v * 5) % 23) / 32.0).astype(np.float32)
    f2 = np.where((u + v) % 31 == 0, 0, 640 + 32 * ((u * 3 + v * 11) % 27)).astype(np.uint16)
    i = np.arange(50)
    pts = np.stack([((i * 7) % 19 - 9) / 16.0 + 1.0 / 256, ((i * 5) % 17 - 8) / 16.0 + 1.0 / 512, ((i * 3) % 13) / 16.0 + 3.0 / 1024], axis=1)
    want = []

    def record(st):
        want.append(np.array([st[k] for k in ("returns", "inside", "occupied_before", "occupied_after")], dtype=np.float64))
        want.append(s.collision_occupancy().astype(np.float64).ravel())
        want.append(s.collision_grid()["G"].astype(np.float64).ravel())
        want.append(s.clearance()["min"])

    record(s.integrate_depth(f1, cam, dims, origin, voxel, filter_q=2, filter_pad=0.0625))
    record(s.integrate_depth(f2, dict(cam, depth_scale=1.0 / 1024), dims, origin, voxel, mode="fuse", carve=True, filter_q=qa[:3], filter_pad=0.0625))
    record(s.integrate_points(pts, dims, origin, voxel, mode="fuse", filter_q=1, filter_pad=0.0))
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert want[1] > 0 and want[3] > 0
