"""CPU: the task interface (include/loik_amd_tasks.h) -- the header declares exactly its five entry points, the library exports
them, the binding's list and version match, and none of it leaks into the lists of the older headers."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_tasks_version", "loikb_pose_set_tasks", "loikb_pose_clear_tasks", "loikb_pose_get_tasks", "loikb_frame_placements"}


def tasks_symbols():
    text = open(os.path.join(ROOT, "include", "loik_amd_tasks.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_the_five_entry_points():
    assert tasks_symbols() == WANT


def test_library_exports_every_tasks_symbol():
    L = loik_amd.lib()
    decl = tasks_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.TASKS_SYMBOLS), decl ^ set(capi.TASKS_SYMBOLS)
    assert not decl & set(capi.EXPORTED_SYMBOLS)
    assert not decl & set(capi.POSE_SYMBOLS)
    assert not decl & set(capi.LIMITS_SYMBOLS)


def test_versions_and_kinds_agree():
    L = loik_amd.lib()
    assert L.loikb_tasks_version() == capi.TASKS_ABI_VERSION == 1
    text = open(os.path.join(ROOT, "include", "loik_amd_tasks.h")).read()
    assert re.search(r"#define LOIKB_TASKS_VERSION 1\b", text)
    assert re.search(r"LOIKB_TASK_POSE = %d, LOIKB_TASK_POSITION = %d, LOIKB_TASK_ORIENTATION = %d\b"
                     % (capi.TASK_POSE, capi.TASK_POSITION, capi.TASK_ORIENTATION), text)
    assert capi.TASK_KINDS == {"pose": 0, "position": 1, "orientation": 2}


def test_older_headers_and_lists_are_untouched():
    """the base, pose and limits headers keep their versions and their symbol counts (tests/test_capi_abi.py, test_pose_abi.py and
    test_limits_abi.py pin them: this says why the tasks live in a header of their own)"""
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_limits_version() == capi.LIMITS_ABI_VERSION == 1 and len(capi.LIMITS_SYMBOLS) == 4
    for header in ("loik_amd.h", "loik_amd_pose.h", "loik_amd_limits.h"):
        assert "loik_amd_tasks" not in open(os.path.join(ROOT, "include", header)).read()
