"""CPU: the Jacobian / dexterity interface (include/loik_amd_jacobian.h) -- the header declares exactly its five entry points, the
library exports them, the binding's list, version and enum values match, and none of it leaks into the lists of the older headers."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_jacobian_version", "loikb_frame_jacobians", "loikb_frame_dexterity", "loikb_dexterity_set_multistart_pick",
        "loikb_dexterity_get_multistart_pick"}


def _header(name="loik_amd_jacobian.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def jacobian_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert jacobian_symbols() == WANT
    # ... and the one type they take
    assert re.search(r"typedef struct loikb_dexterity_params \{.*?\} loikb_dexterity_params;", _header(), flags=re.S)


def test_library_exports_every_jacobian_symbol():
    L = loik_amd.lib()
    decl = jacobian_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.JACOBIAN_SYMBOLS), decl ^ set(capi.JACOBIAN_SYMBOLS)
    assert len(capi.JACOBIAN_SYMBOLS) == 5
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS,
                  capi.PATH_SYMBOLS, capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS):
        assert not decl & set(older)


def test_versions_and_enums_agree():
    L = loik_amd.lib()
    assert L.loikb_jacobian_version() == capi.JACOBIAN_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_JACOBIAN_VERSION 1\b", text)
    assert re.search(r"LOIKB_JAC_LOCAL = %d, LOIKB_JAC_LOCAL_WORLD_ALIGNED = %d, LOIKB_JAC_WORLD = %d\b"
                     % (capi.JAC_LOCAL, capi.JAC_LOCAL_WORLD_ALIGNED, capi.JAC_WORLD), text)
    assert (capi.JAC_LOCAL, capi.JAC_LOCAL_WORLD_ALIGNED, capi.JAC_WORLD) == (0, 1, 2)
    assert capi.JAC_REFERENCES == {"local": 0, "local_world_aligned": 1, "world": 2}
    for k in range(6):
        assert re.search(r"LOIKB_DEX_SIGMA%d = %d\b" % (k, capi.DEX_SIGMA0 + k), text)
    assert re.search(r"LOIKB_DEX_MANIPULABILITY = %d, LOIKB_DEX_INV_CONDITION = %d, LOIKB_DEX_N = %d\b"
                     % (capi.DEX_MANIPULABILITY, capi.DEX_INV_CONDITION, capi.DEX_N), text)
    assert (capi.DEX_SIGMA0, capi.DEX_MANIPULABILITY, capi.DEX_INV_CONDITION, capi.DEX_N) == (0, 6, 7, 8)
    # the struct of the binding has the header's members in the header's order
    members = re.findall(r"^\s*(?:double|int)\s+([a-z_]+);",
                         re.search(r"typedef struct loikb_dexterity_params \{(.*?)\} loikb_dexterity_params;", text, flags=re.S).group(1), flags=re.M)
    assert members == [f[0] for f in capi.DexterityParams._fields_] == ["length", "flags"]


def test_binding_and_mirror_have_the_methods():
    for name in ("frame_jacobians", "frame_dexterity", "set_multistart_pick_dexterous", "clear_multistart_pick_dexterous",
                 "multistart_pick_dexterous"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_jacobian.h"' in mirror
    for name in ("FrameJacobians", "FrameDexterity", "TaskDexterity", "setMultiStartPickDexterous", "clearMultiStartPickDexterous"):
        assert re.search(r"\b%s\(" % name, mirror), name


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_tasks_version() == capi.TASKS_ABI_VERSION == 1 and len(capi.TASKS_SYMBOLS) == 5
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_step_version() == capi.STEP_ABI_VERSION == 1 and len(capi.STEP_SYMBOLS) == 4
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert capi.MS_PICKS == {"nearest": 0, "first": 1}
    # the multi-start header says nothing of the new pick: it is this header's
    assert "dexter" not in _header("loik_amd_multistart.h").lower()
