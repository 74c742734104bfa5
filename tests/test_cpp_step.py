"""The step-control layer of the C++ mirror (include/loik_amd/loik.hpp: setStepControl, clearStepControl, PoseResult::alpha /
backtracks / failed) compiles against include/loik_amd_step.h and links (CPU); tests/cpp/test_step.cpp runs the rescue and the stall
case on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_step_mirror_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_step.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_step")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_step_mirror_runs():
    test_cpp_step_mirror_compiles()
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_step")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all step checks passed" in out.stdout, out.stdout + out.stderr
