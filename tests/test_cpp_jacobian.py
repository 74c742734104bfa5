"""The Jacobian / dexterity calls through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_jacobian.h) compile
and link (CPU); tests/cpp/test_jacobian.cpp runs on the GPU, and what its three calls return is what the Python binding returns, bit for
bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_jacobian_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_jacobian.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_jacobian")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_jacobian_runs_and_matches_the_binding(tmp_path):
    import loik_amd
    from test_pose_ik import _handle
    test_cpp_jacobian_compiles()
    dump = str(tmp_path / "jacobian.bin")
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_jacobian"), dump], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all jacobian checks passed" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(dump, dtype=np.float64)
    # the same calls through the binding, on the same configurations (sixteenths: the same doubles in both languages)
    model = loik_amd.builtin_model("panda7")
    B = 67
    q0 = np.array([[((b * 7 + 3 * k) % 17 - 8) / 16.0 for k in range(model.nq)] for b in range(B)])
    tool = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, 0.125, 0.0, 0.25], dtype=float)
    elbow = np.array([1, 0, 0, 0, 0, -1, 0, 1, 0, 0.0, 0.5, 0.0], dtype=float)
    s, _ = _handle(model, B, [7], q0)
    frames = np.stack([tool, elbow])
    want = [s.frame_jacobians([7, 4], frames, reference=r).ravel() for r in ("local", "local_world_aligned", "world")]
    d = s.frame_dexterity([7, 4], frames, [0x3f, 0x07], length=0.5)
    want.append(np.concatenate([d["sigma"], d["manipulability"][..., None], d["inv_condition"][..., None]], axis=2).ravel())
    s.set_pose_tasks(["position"], tool[None])
    d = s.frame_dexterity(length=0.5)
    want.append(np.concatenate([d["sigma"], d["manipulability"][..., None], d["inv_condition"][..., None]], axis=2).ravel())
    s.close()
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
