"""CPU: the shortcut interface (include/loik_amd_shortcut.h) -- the header declares exactly its three entry points, the library exports
them, the binding's list, version and struct match, the mirror names them, and none of it leaks into the older headers and lists."""
import ctypes as C
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_shortcut_version", "loikb_shortcut_paths", "loikb_path_length"}


def _header(name="loik_amd_shortcut.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def shortcut_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert shortcut_symbols() == WANT
    assert re.search(r"typedef struct loikb_shortcut_params \{.*?\} loikb_shortcut_params;", _header(), flags=re.S)
    assert '#include "loik_amd_motion.h"' in _header()
    assert "never certifies a segment of the input" in _header() and "not guaranteed" in _header()


def test_library_exports_every_shortcut_symbol():
    L = loik_amd.lib()
    decl = shortcut_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.SHORTCUT_SYMBOLS), decl ^ set(capi.SHORTCUT_SYMBOLS)
    assert len(capi.SHORTCUT_SYMBOLS) == 3
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PATH_SYMBOLS,
                  capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS, capi.JACOBIAN_SYMBOLS, capi.COLLISION_SYMBOLS,
                  capi.MOTION_SYMBOLS, capi.AVOID_SYMBOLS):
        assert not decl & set(older)


def test_version_and_struct_agree():
    L = loik_amd.lib()
    assert L.loikb_shortcut_version() == capi.SHORTCUT_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_SHORTCUT_VERSION 1\b", text)
    body = re.search(r"typedef struct loikb_shortcut_params \{(.*?)\} loikb_shortcut_params;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(double|int|unsigned long long)\s+([a-z_]+);", body, flags=re.M)
    assert [m[1] for m in members] == [f[0] for f in capi.ShortcutParams._fields_] == ["margin", "tol", "max_evals", "rounds", "seed", "flags"]
    assert [m[0] for m in members] == ["double", "double", "int", "int", "unsigned long long", "int"]
    ctype = {"double": C.c_double, "int": C.c_int, "unsigned long long": C.c_ulonglong}
    assert [ctype[m[0]] for m in members] == [f[1] for f in capi.ShortcutParams._fields_]
    assert C.sizeof(capi.ShortcutParams) == 40 and capi.ShortcutParams.seed.offset == 24


def test_binding_and_mirror_have_the_methods():
    for name in ("shortcut_paths", "path_length"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_shortcut.h"' in mirror
    for name in ("ShortcutPaths", "PathLength"):
        assert re.search(r"\b%s\(" % name, mirror), name
    for sym in WANT - {"loikb_shortcut_version"}:
        assert sym + "(" in mirror, sym


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_avoid_version() == capi.AVOID_ABI_VERSION == 1 and len(capi.AVOID_SYMBOLS) == 6
    assert L.loikb_motion_version() == capi.MOTION_ABI_VERSION == 1 and len(capi.MOTION_SYMBOLS) == 4
    assert L.loikb_collision_version() == capi.COLLISION_ABI_VERSION == 1 and len(capi.COLLISION_SYMBOLS) == 9
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_path_version() == capi.PATH_ABI_VERSION == 1 and len(capi.PATH_SYMBOLS) == 3
    assert L.loikb_version() == capi.ABI_VERSION == 602
    for older in ("loik_amd_avoid.h", "loik_amd_motion.h", "loik_amd_collision.h", "loik_amd_multistart.h", "loik_amd_path.h", "loik_amd_pose.h",
                  "loik_amd_limits.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "loikb_shortcut" not in text and "loikb_path_length" not in text and "loik_amd_shortcut" not in text
