"""CPU: the blend interface (include/loik_amd_blend.h) -- the header declares exactly its two entry points, the library exports them, the
binding's list, version, struct and enums match, the mirror names the methods, the header says what it must about the certificate, and
none of it leaks into the older headers and lists; loik_amd_retime.h is the text it was."""
import ctypes as C
import hashlib
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_blend_version", "loikb_blend_paths"}
MEMBERS = ["margin", "tol", "reach", "dt", "max_evals", "max_tries", "flags"]
STATUSES = ("TAKEN", "BLOCKED", "UNDECIDED", "COUPLED", "ZERO_LEG", "OFF")


def _header(name="loik_amd_blend.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def blend_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert blend_symbols() == WANT
    assert re.search(r"typedef struct loikb_blend_params \{.*?\} loikb_blend_params;", _header(), flags=re.S)
    assert '#include "loik_amd_retime.h"' in _header()
    # what the header must state
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    for phrase in ("sub-interval of an input segment", "this call does not check those", "they are certified if the input was",
                   "a blend curve that this call certified at a clearance >= margin", "agree to rounding, not bit for bit",
                   "The result is not time-optimal", "the fastest trajectory on this geometry with blends traversed at a constant rate",
                   "There is no SNAP in this version", "A call that fails writes nothing"):
        assert phrase in text, phrase
    assert "is time-optimal" not in text and "LOIKB_BLEND_SNAP" not in text


def test_library_exports_every_blend_symbol():
    L = loik_amd.lib()
    decl = blend_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.BLEND_SYMBOLS), decl ^ set(capi.BLEND_SYMBOLS)
    assert len(capi.BLEND_SYMBOLS) == 2
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PATH_SYMBOLS,
                  capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS, capi.JACOBIAN_SYMBOLS, capi.COLLISION_SYMBOLS,
                  capi.MOTION_SYMBOLS, capi.AVOID_SYMBOLS, capi.SHORTCUT_SYMBOLS, capi.RETIME_SYMBOLS, capi.PLAN_SYMBOLS):
        assert not decl & set(older)


def test_version_struct_and_enums_agree():
    L = loik_amd.lib()
    assert L.loikb_blend_version() == capi.BLEND_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_BLEND_VERSION 1\b", text)
    body = re.search(r"typedef struct loikb_blend_params \{(.*?)\} loikb_blend_params;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(double|int)\s+([a-z_]+);", body, flags=re.M)
    assert [m[1] for m in members] == [f[0] for f in capi.BlendParams._fields_] == MEMBERS
    assert [m[0] for m in members] == ["double"] * 4 + ["int"] * 3
    ctype = {"double": C.c_double, "int": C.c_int}
    assert [ctype[m[0]] for m in members] == [f[1] for f in capi.BlendParams._fields_]
    # four doubles, three ints and the padding behind them
    assert C.sizeof(capi.BlendParams) == 48
    assert [getattr(capi.BlendParams, m).offset for m in MEMBERS] == [0, 8, 16, 24, 32, 36, 40]
    names = re.search(r"enum \{(.*?)\};", text, flags=re.S).group(1)
    assert dict((k, int(v)) for k, v in re.findall(r"LOIKB_BLEND_([A-Z_]+) = (\d+)", names)) == {k: getattr(capi, "BLEND_" + k) for k in STATUSES}
    assert [getattr(capi, "BLEND_" + k) for k in STATUSES] == list(range(6))
    for name, value in (("TRUNCATED", capi.BLEND_TRUNCATED), ("INVALID", capi.BLEND_INVALID), ("SKIPPED", capi.BLEND_SKIPPED)):
        assert re.search(r"#define LOIKB_BLEND_%s %d\b" % (name, value), text), name
    assert (capi.BLEND_TRUNCATED, capi.BLEND_INVALID, capi.BLEND_SKIPPED) == (capi.RETIME_TRUNCATED, capi.RETIME_INVALID, capi.RETIME_SKIPPED) == (1, 2, 4)


def test_binding_and_mirror_have_the_methods():
    assert callable(getattr(loik_amd.BatchedLoik, "blend_paths"))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_blend.h"' in mirror
    for name in (r"BlendPaths\(", r"struct BlendResult\b"):
        assert re.search(r"\b%s" % name, mirror), name
    assert "loikb_blend_paths(" in mirror
    build = open(os.path.join(ROOT, "loik_amd", "_build.py")).read()
    assert "loik_amd_blend.h" in build and "loik_pose_blend.hpp" in build


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_plan_version() == capi.PLAN_ABI_VERSION == 1 and len(capi.PLAN_SYMBOLS) == 2
    assert L.loikb_retime_version() == capi.RETIME_ABI_VERSION == 1 and len(capi.RETIME_SYMBOLS) == 2
    assert L.loikb_shortcut_version() == capi.SHORTCUT_ABI_VERSION == 1 and len(capi.SHORTCUT_SYMBOLS) == 3
    assert L.loikb_motion_version() == capi.MOTION_ABI_VERSION == 1 and len(capi.MOTION_SYMBOLS) == 4
    assert L.loikb_version() == capi.ABI_VERSION == 602
    for older in ("loik_amd_plan.h", "loik_amd_retime.h", "loik_amd_shortcut.h", "loik_amd_avoid.h", "loik_amd_motion.h", "loik_amd_collision.h",
                  "loik_amd_multistart.h", "loik_amd_path.h", "loik_amd_pose.h", "loik_amd_limits.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "loikb_blend" not in text and "loik_amd_blend" not in text
    # loik_amd_retime.h byte for byte
    assert hashlib.sha256(open(os.path.join(ROOT, "include", "loik_amd_retime.h"), "rb").read()).hexdigest() == \
        "f0a151b492592de376889757d630ea806ea7e51027f42e82948be8365e8d486a"
