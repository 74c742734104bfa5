"""CPU: the step-control interface (include/loik_amd_step.h) -- the header declares exactly its entry points, the library exports
them, the binding's list, version and enum values match, none of it leaks into the lists of the older headers, and the STALLED
bit is a fifth bit of the pose status word."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_step_version", "loikb_pose_set_step_control", "loikb_pose_get_step_control", "loikb_step_get"}


def _header(name="loik_amd_step.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def step_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert step_symbols() == WANT
    # ... and the one type they take
    assert re.search(r"typedef struct loikb_step_params \{.*?\} loikb_step_params;", _header(), flags=re.S)


def test_library_exports_every_step_symbol():
    L = loik_amd.lib()
    decl = step_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.STEP_SYMBOLS), decl ^ set(capi.STEP_SYMBOLS)
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS,
                  capi.PATH_SYMBOLS, capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS):
        assert not decl & set(older)


def test_versions_and_enums_agree():
    L = loik_amd.lib()
    assert L.loikb_step_version() == capi.STEP_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_STEP_VERSION 1\b", text)
    assert re.search(r"LOIKB_POSE_ST_STALLED = %d\b" % capi.POSE_ST_STALLED, text)
    assert re.search(r"LOIKB_STEP_F_ALPHA = %d,[^;]*LOIKB_STEP_F_BACKTRACKS,[^;]*LOIKB_STEP_F_FAILED\b" % capi.STEP_F_ALPHA, text, flags=re.S)
    assert (capi.STEP_F_ALPHA, capi.STEP_F_BACKTRACKS, capi.STEP_F_FAILED) == (0, 1, 2)
    # the struct of the binding has the header's members in the header's order
    members = re.findall(r"^\s*(?:double|int)\s+([a-z_]+);", re.search(r"typedef struct loikb_step_params \{(.*?)\} loikb_step_params;", text, flags=re.S).group(1), flags=re.M)
    assert members == [f[0] for f in capi.StepParams._fields_] == ["shrink", "sufficient", "max_backtracks", "patience", "flags"]


def test_stalled_is_a_fifth_status_bit():
    bits = [capi.POSE_ST_REACHED, capi.POSE_ST_NOT_CONVERGED, capi.POSE_ST_INFEASIBLE, capi.POSE_ST_STOPPED, capi.POSE_ST_STALLED]
    assert capi.POSE_ST_STALLED == 16 and len(set(bits)) == 5
    assert all(b > 0 and b & (b - 1) == 0 for b in bits)
    pose = _header("loik_amd_pose.h")
    for name, b in zip(("REACHED", "NOT_CONVERGED", "INFEASIBLE", "STOPPED"), bits):
        assert re.search(r"LOIKB_POSE_ST_%s = %d\b" % (name, b), pose)
    assert "STALLED" not in pose


def test_binding_has_the_methods():
    for name in ("set_step_control", "clear_step_control", "step_control", "step_get"):
        assert callable(getattr(loik_amd.BatchedLoik, name))


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_limits_version() == capi.LIMITS_ABI_VERSION == 1 and len(capi.LIMITS_SYMBOLS) == 4
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_accel_version() == capi.ACCEL_ABI_VERSION == 1 and len(capi.ACCEL_SYMBOLS) == 4
    assert L.loikb_version() == capi.ABI_VERSION == 602
