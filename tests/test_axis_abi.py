"""CPU: the axis-task interface (include/loik_amd_axis.h) -- the header declares exactly its one entry point, the library exports
it, the binding's list, version and kinds match, the tasks header and the binding's TASK_KINDS are what they were, and the older
headers do not know the new one."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_axis_version"}
OLDER_HEADERS = ("loik_amd.h", "loik_amd_models.h", "loik_amd_pose.h", "loik_amd_limits.h", "loik_amd_tasks.h", "loik_amd_multistart.h",
                 "loik_amd_path.h", "loik_amd_track.h", "loik_amd_accel.h")


def _header(name="loik_amd_axis.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def axis_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_the_one_entry_point():
    assert axis_symbols() == WANT
    assert re.search(r'#include "loik_amd_tasks.h"', _header())


def test_library_exports_the_axis_symbol():
    L = loik_amd.lib()
    decl = axis_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.AXIS_SYMBOLS), decl ^ set(capi.AXIS_SYMBOLS)
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS,
                  capi.PATH_SYMBOLS, capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS):
        assert not decl & set(older)


def test_version_and_kinds_agree():
    L = loik_amd.lib()
    assert L.loikb_axis_version() == capi.AXIS_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_AXIS_VERSION 1\b", text)
    assert re.search(r"LOIKB_TASK_FREE_Z = %d\b" % capi.TASK_FREE_Z, text)
    assert re.search(r"LOIKB_TASK_POSE_AXIS = LOIKB_TASK_POSE \| LOIKB_TASK_FREE_Z\b", text)
    assert re.search(r"LOIKB_TASK_AXIS = LOIKB_TASK_ORIENTATION \| LOIKB_TASK_FREE_Z\b", text)
    assert (capi.TASK_FREE_Z, capi.TASK_POSE_AXIS, capi.TASK_AXIS) == (4, 4, 6)
    assert capi.TASK_POSE_AXIS == capi.TASK_POSE | capi.TASK_FREE_Z and capi.TASK_AXIS == capi.TASK_ORIENTATION | capi.TASK_FREE_Z
    assert capi.AXIS_TASK_KINDS == {"pose_axis": 4, "axis": 6}
    # the tasks header's own table keeps its three names
    assert capi.TASK_KINDS == {"pose": 0, "position": 1, "orientation": 2}
    assert not set(capi.AXIS_TASK_KINDS) & set(capi.TASK_KINDS)


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_tasks_version() == capi.TASKS_ABI_VERSION == 1 and len(capi.TASKS_SYMBOLS) == 5
    assert L.loikb_track_version() == capi.TRACK_ABI_VERSION == 1 and len(capi.TRACK_SYMBOLS) == 3
    assert L.loikb_accel_version() == capi.ACCEL_ABI_VERSION == 1 and len(capi.ACCEL_SYMBOLS) == 4
    for header in OLDER_HEADERS:
        assert "loik_amd_axis" not in _header(header), header
    assert re.search(r"enum \{ LOIKB_TASK_POSE = 0, LOIKB_TASK_POSITION = 1, LOIKB_TASK_ORIENTATION = 2 \};", _header("loik_amd_tasks.h"))
