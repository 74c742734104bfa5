"""The owning buffer type of the host layer (loik_amd/csrc/loik_devmem.hpp) on the CPU: tests/cpp/test_devmem.cpp instantiates it over
a counting malloc-backed policy and runs as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_owner_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_devmem.cpp")
    exe = str(tmp_path / "test_devmem")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "all devmem checks passed" in out.stdout, out.stdout + out.stderr
