"""CPU: the batched pose IK interface (include/loik_amd_pose.h) -- the library exports what the header declares, the binding's
list and version match, the numpy log6 of the tests inverts exp6 over the whole range, and the C++ mirror with SolvePose compiles."""
import os
import re
import subprocess

import numpy as np
import pytest

import loik_amd
from loik_amd import capi

import pose_numpy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pose_symbols():
    text = open(os.path.join(ROOT, "include", "loik_amd_pose.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_library_exports_every_pose_symbol():
    L = loik_amd.lib()
    decl = pose_symbols()
    assert len(decl) == 4
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.POSE_SYMBOLS), decl ^ set(capi.POSE_SYMBOLS)
    assert not decl & set(capi.EXPORTED_SYMBOLS)
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1
    text = open(os.path.join(ROOT, "include", "loik_amd_pose.h")).read()
    assert re.search(r"#define LOIKB_POSE_VERSION 1\b", text)
    assert re.search(r"LOIKB_POSE_TARGET_SHARED = %d\b" % capi.POSE_TARGET_SHARED, text)


@pytest.mark.parametrize("theta", [0.0, 1e-12, 1e-8, 1e-5, 1e-3, 1.0, 2.5, np.pi - 1e-3, np.pi - 1e-6])
def test_numpy_log6_inverts_exp6(theta):
    rng = np.random.default_rng(int(theta * 1e6) % 1000)
    for _ in range(50):
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        nu = np.r_[rng.normal(size=3), theta * a]
        R, p = P.exp6(nu)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14)
        assert np.max(np.abs(P.log6(R, p) - nu)) < 1e-12


def test_numpy_fk_matches_oracle_placements():
    """the tests' FK agrees with the CPU oracle's data.oMi (one more independent restatement)"""
    from oracle import ref
    m = loik_amd.builtin_model("talos32")
    q = m.random_configurations(np.random.default_rng(3), 4)
    r = ref.RefSolver(m, max_iter=5)
    for b in range(4):
        r.SolveInit(q[b], np.eye(6), np.zeros(6), np.array([21], dtype=np.int32), np.eye(6)[None], np.zeros((1, 6)),
                    -np.ones(m.nv), np.ones(m.nv))
        assert np.max(np.abs(r.field("oMi")[1:] - P.fk12(m, q[b:b + 1], range(1, m.njoints))[0])) < 1e-13


def test_cpp_pose_mirror_compiles():
    """loik.hpp's SolvePose / ForwardKinematics compile against the header and link (as tests/cpp is built)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_pose.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_pose")
    libdir = os.path.join(ROOT, "loik_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", libdir, "-lloik_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_pose_mirror_runs():
    test_cpp_pose_mirror_compiles()
    out = subprocess.run([os.path.join(ROOT, "tests", "cpp", "test_pose")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all pose checks passed" in out.stdout, out.stdout + out.stderr
