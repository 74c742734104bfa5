"""CPU: the retiming interface (include/loik_amd_retime.h) -- the header declares exactly its two entry points, the library exports them,
the binding's list, version and struct match, the mirror names them, and none of it leaks into the older headers and lists."""
import ctypes as C
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_retime_version", "loikb_retime_paths"}


def _header(name="loik_amd_retime.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def retime_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert retime_symbols() == WANT
    assert re.search(r"typedef struct loikb_retime_params \{.*?\} loikb_retime_params;", _header(), flags=re.S)
    assert '#include "loik_amd_motion.h"' in _header()
    # what the header must state
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    for phrase in ("Every sample lies on a segment of the input", "stays certified", "time-optimal among those that follow the path exactly",
                   "stops at every waypoint", "Corner blending leaves the certified geometry and is out of scope"):
        assert phrase in text, phrase


def test_library_exports_every_retime_symbol():
    L = loik_amd.lib()
    decl = retime_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.RETIME_SYMBOLS), decl ^ set(capi.RETIME_SYMBOLS)
    assert len(capi.RETIME_SYMBOLS) == 2
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PATH_SYMBOLS,
                  capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS, capi.JACOBIAN_SYMBOLS, capi.COLLISION_SYMBOLS,
                  capi.MOTION_SYMBOLS, capi.AVOID_SYMBOLS, capi.SHORTCUT_SYMBOLS):
        assert not decl & set(older)


def test_version_struct_and_flags_agree():
    L = loik_amd.lib()
    assert L.loikb_retime_version() == capi.RETIME_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_RETIME_VERSION 1\b", text)
    body = re.search(r"typedef struct loikb_retime_params \{(.*?)\} loikb_retime_params;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(double|int)\s+([a-z_]+);", body, flags=re.M)
    assert [m[1] for m in members] == [f[0] for f in capi.RetimeParams._fields_] == ["dt", "flags"]
    ctype = {"double": C.c_double, "int": C.c_int}
    assert [ctype[m[0]] for m in members] == [f[1] for f in capi.RetimeParams._fields_]
    assert C.sizeof(capi.RetimeParams) == 16 and capi.RetimeParams.flags.offset == 8
    for name, value in (("SNAP", capi.RETIME_SNAP), ("TRUNCATED", capi.RETIME_TRUNCATED), ("INVALID", capi.RETIME_INVALID), ("SKIPPED", capi.RETIME_SKIPPED)):
        assert re.search(r"#define LOIKB_RETIME_%s %d\b" % (name, value), text), name
    assert (capi.RETIME_SNAP, capi.RETIME_TRUNCATED, capi.RETIME_INVALID, capi.RETIME_SKIPPED) == (1, 1, 2, 4)


def test_binding_and_mirror_have_the_method():
    assert callable(getattr(loik_amd.BatchedLoik, "retime_paths"))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_retime.h"' in mirror
    assert re.search(r"\bRetimePaths\(", mirror) and "loikb_retime_paths(" in mirror


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_shortcut_version() == capi.SHORTCUT_ABI_VERSION == 1 and len(capi.SHORTCUT_SYMBOLS) == 3
    assert L.loikb_avoid_version() == capi.AVOID_ABI_VERSION == 1 and len(capi.AVOID_SYMBOLS) == 6
    assert L.loikb_motion_version() == capi.MOTION_ABI_VERSION == 1 and len(capi.MOTION_SYMBOLS) == 4
    assert L.loikb_collision_version() == capi.COLLISION_ABI_VERSION == 1 and len(capi.COLLISION_SYMBOLS) == 9
    assert L.loikb_path_version() == capi.PATH_ABI_VERSION == 1 and len(capi.PATH_SYMBOLS) == 3
    assert L.loikb_version() == capi.ABI_VERSION == 602
    for older in ("loik_amd_shortcut.h", "loik_amd_avoid.h", "loik_amd_motion.h", "loik_amd_collision.h", "loik_amd_multistart.h", "loik_amd_path.h",
                  "loik_amd_pose.h", "loik_amd_limits.h", "loik_amd_accel.h", "loik_amd_track.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "loikb_retime" not in text and "loik_amd_retime" not in text
