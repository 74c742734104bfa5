"""The axis-symmetric task kinds through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_axis.h)
compile and link (CPU); tests/cpp/test_axis_tasks.cpp runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_axis_tasks_compiles():
    import loik_amd
    loik_amd.lib()
    src = os.path.join(ROOT, "tests", "cpp", "test_axis_tasks.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_axis_tasks")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_axis_tasks_runs():
    test_cpp_axis_tasks_compiles()
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_axis_tasks")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all axis tasks checks passed" in out.stdout, out.stdout + out.stderr
