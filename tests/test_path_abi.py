"""CPU: the path interface (include/loik_amd_path.h) -- the header declares exactly its three entry points, the library exports
them, the binding's list, version, enums and struct match, and none of it leaks into the older headers and their lists."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_path_version", "loikb_solve_pose_path", "loikb_path_get"}
OLDER = {"loik_amd_pose.h": "POSE_SYMBOLS", "loik_amd_limits.h": "LIMITS_SYMBOLS", "loik_amd_tasks.h": "TASKS_SYMBOLS",
         "loik_amd_multistart.h": "MULTISTART_SYMBOLS"}


def header_symbols(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_the_three_entry_points():
    assert header_symbols("loik_amd_path.h") == WANT == set(capi.PATH_SYMBOLS)


def test_library_exports_every_path_symbol():
    L = loik_amd.lib()
    for name in WANT:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS):
        assert not WANT & set(older)


def test_version_enums_and_struct_agree():
    L = loik_amd.lib()
    assert L.loikb_path_version() == capi.PATH_ABI_VERSION == 1
    text = open(os.path.join(ROOT, "include", "loik_amd_path.h")).read()
    assert re.search(r"#define LOIKB_PATH_VERSION 1\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fields = re.findall(r"\bLOIKB_PATH_F_([A-Z_]+)", code)
    assert fields == ["CURSOR", "STATUS", "WSTEPS", "Q", "TIMING"]
    assert [getattr(capi, "PATH_F_" + f) for f in fields] == list(range(5))
    assert re.search(r"LOIKB_PATH_ST_COMPLETE = %d," % capi.PATH_ST_COMPLETE, code) and capi.PATH_ST_COMPLETE == 1
    assert re.search(r"LOIKB_PATH_ST_STALLED = %d\b" % capi.PATH_ST_STALLED, code) and capi.PATH_ST_STALLED == 2
    body = re.search(r"typedef struct loikb_path_params \{(.*?)\} loikb_path_params;", code, flags=re.S).group(1)
    names = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in capi.PathParams._fields_] == ["n_waypoints", "max_steps_per_waypoint", "record", "flags"]


def test_older_headers_and_lists_are_untouched():
    """the base, pose, limits, tasks and multi-start headers keep their versions and their symbol sets: the path lives in a header
    of its own"""
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_limits_version() == capi.LIMITS_ABI_VERSION == 1 and len(capi.LIMITS_SYMBOLS) == 4
    assert L.loikb_tasks_version() == capi.TASKS_ABI_VERSION == 1 and len(capi.TASKS_SYMBOLS) == 5
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    for header, listed in OLDER.items():
        assert header_symbols(header) == set(getattr(capi, listed)), header
        assert "loikb_path" not in open(os.path.join(ROOT, "include", header)).read(), header
    base = header_symbols("loik_amd.h") | header_symbols("loik_amd_models.h")
    assert base == set(capi.EXPORTED_SYMBOLS) and "loikb_path" not in open(os.path.join(ROOT, "include", "loik_amd.h")).read()
