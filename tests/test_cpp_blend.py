"""The blend call through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_blend.h) compiles and links (CPU);
tests/cpp/test_blend.cpp runs on the GPU, and what its BlendPaths calls return is what the Python binding returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from test_cpp_motion import cpp_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_blend_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_blend.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_blend")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_blend_runs_and_matches_the_binding(tmp_path):
    from test_pose_ik import _handle
    test_cpp_blend_compiles()
    dump = str(tmp_path / "blend.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_blend"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all blend checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    model, qa, _, links, spheres, ws, box = cpp_case()
    B, T = qa.shape[0], 4
    paths = np.ascontiguousarray(qa[:B // T * T].reshape(B // T, T, model.nq))
    j = np.arange(model.nv)
    kw = dict(v_max=1.0 + j / 8.0, a_max=2.0 + j / 4.0, dt=1.0 / 32, reach=0.25, margin=-0.0625, tol=1.0 / 1024, max_evals=16, max_tries=3)
    n = np.arange(B // T, dtype=np.int32) % (T + 2)
    s, _ = _handle(model, B, [7], qa)
    s.set_collision_spheres(links, spheres)
    s.set_collision_world(ws, [box])
    s.set_self_collision(True, ignore=[(2, 4)])
    want = []
    for r in (s.blend_paths(paths, **kw), s.blend_paths(paths, n_waypoints=n, max_samples=64, **kw), s.blend_paths(paths, max_samples=0, **kw)):
        rows = 0 if r["q_traj"] is None else r["q_traj"].shape[1]
        want.append(np.array([float(rows)]))
        want += [r[k].astype(np.float64).ravel() for k in ("q_traj", "v_traj") if r[k] is not None]
        want += [r[k].astype(np.float64).ravel() for k in ("n_samples", "n_waypoints", "taken", "flags", "duration", "corner", "corner_info", "piece")]
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
