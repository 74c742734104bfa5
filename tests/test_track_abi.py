"""CPU: the tracking interface (include/loik_amd_track.h) -- the header declares exactly its three entry points, the library
exports them, the binding's list, version, enums and struct match, and none of it leaks into the older headers and their lists."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_track_version", "loikb_track_pose", "loikb_track_get"}
OLDER = {"loik_amd_pose.h": "POSE_SYMBOLS", "loik_amd_limits.h": "LIMITS_SYMBOLS", "loik_amd_tasks.h": "TASKS_SYMBOLS",
         "loik_amd_multistart.h": "MULTISTART_SYMBOLS", "loik_amd_path.h": "PATH_SYMBOLS"}


def header_symbols(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_the_three_entry_points():
    assert header_symbols("loik_amd_track.h") == WANT == set(capi.TRACK_SYMBOLS)


def test_library_exports_every_track_symbol():
    L = loik_amd.lib()
    for name in WANT:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PATH_SYMBOLS):
        assert not WANT & set(older)


def test_version_enums_and_struct_agree():
    L = loik_amd.lib()
    assert L.loikb_track_version() == capi.TRACK_ABI_VERSION == 1
    text = open(os.path.join(ROOT, "include", "loik_amd_track.h")).read()
    assert re.search(r"#define LOIKB_TRACK_VERSION 1\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    fields = re.findall(r"\bLOIKB_TRACK_F_([A-Z_]+)", code)
    assert fields == ["Q", "Z", "ERRMAX", "INNER", "ONTRACK", "WORST", "WORST_AT", "TIMING"]
    assert [getattr(capi, "TRACK_F_" + f) for f in fields] == list(range(8))
    assert re.search(r"LOIKB_TRACK_F_Q = 0,", code)
    assert re.search(r"LOIKB_TRACK_FF_NONE = %d," % capi.TRACK_FF_NONE, code) and capi.TRACK_FF_NONE == 0
    assert re.search(r"LOIKB_TRACK_FF_DIFFERENCE = %d\b" % capi.TRACK_FF_DIFFERENCE, code) and capi.TRACK_FF_DIFFERENCE == 1
    assert re.search(r"LOIKB_TRACK_REC_Q = %d," % capi.TRACK_REC_Q, code) and capi.TRACK_REC_Q == 1
    assert re.search(r"LOIKB_TRACK_REC_Z = %d\b" % capi.TRACK_REC_Z, code) and capi.TRACK_REC_Z == 2
    body = re.search(r"typedef struct loikb_track_params \{(.*?)\} loikb_track_params;", code, flags=re.S).group(1)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert [d[-1] for d in decls] == [n for n, _ in capi.TrackParams._fields_] == ["dt", "gain", "tol_track", "n_steps", "feedforward", "record", "flags"]
    import ctypes as C
    assert [d[0] for d in decls] == ["double" if t is C.c_double else "int" for _, t in capi.TrackParams._fields_]
    # the binding's table of the getter's fields: every array field, its dimensions as the header documents them, the int ones
    assert set(capi.TRACK_FIELD_ID) == set(capi.TRACK_FIELD_DIMS) and set(capi.TRACK_INT_FIELDS) <= set(capi.TRACK_FIELD_ID)
    assert sorted(capi.TRACK_FIELD_ID.values()) == list(range(7)) and capi.TRACK_F_TIMING == 7
    dims = {"q_traj": "[T+1][nq]", "z_traj": "[T][nv]", "errmax": "[T+1]", "inner": "[T]", "ontrack": "", "worst": "", "worst_at": ""}
    for name, fid in capi.TRACK_FIELD_ID.items():
        line = re.search(r"LOIKB_TRACK_F_%s\b[^\n]*/\* (int|double) \[B\]((?:\[[^\]]+\])*)" % fields[fid], text)
        assert line, name
        assert (line.group(1) == "int") == (name in capi.TRACK_INT_FIELDS), name
        assert line.group(2) == dims[name] == "".join("[%s]" % d for d in capi.TRACK_FIELD_DIMS[name]), name


def test_older_headers_and_lists_are_untouched():
    """the base, pose, limits, tasks, multi-start and path headers keep their versions and their symbol sets: tracking lives in a
    header of its own"""
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_limits_version() == capi.LIMITS_ABI_VERSION == 1 and len(capi.LIMITS_SYMBOLS) == 4
    assert L.loikb_tasks_version() == capi.TASKS_ABI_VERSION == 1 and len(capi.TASKS_SYMBOLS) == 5
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_path_version() == capi.PATH_ABI_VERSION == 1 and len(capi.PATH_SYMBOLS) == 3
    for header, listed in OLDER.items():
        assert header_symbols(header) == set(getattr(capi, listed)), header
        assert "loikb_track" not in open(os.path.join(ROOT, "include", header)).read(), header
    base = header_symbols("loik_amd.h") | header_symbols("loik_amd_models.h")
    assert base == set(capi.EXPORTED_SYMBOLS) and "loikb_track" not in open(os.path.join(ROOT, "include", "loik_amd.h")).read()
    # loikb_get's own table is loikb_get's alone
    assert set(capi.FIELD_DIMS) == set(capi.FIELD_ID) | {"scalars"} and len(capi.INT_FIELDS) == 5
