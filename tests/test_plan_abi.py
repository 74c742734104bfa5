"""CPU: the planning interface (include/loik_amd_plan.h) -- the header declares exactly its two entry points, the library exports them,
the binding's list, version and struct match, the mirror names them, and none of it leaks into the older headers and lists."""
import ctypes as C
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_plan_version", "loikb_plan_paths"}
MEMBERS = ["margin", "tol", "step", "seed", "max_evals", "max_iters", "max_nodes", "flags"]


def _header(name="loik_amd_plan.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def plan_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert plan_symbols() == WANT
    assert re.search(r"typedef struct loikb_plan_params \{.*?\} loikb_plan_params;", _header(), flags=re.S)
    assert '#include "loik_amd_motion.h"' in _header()
    text = " ".join(_header().replace("*", " ").split())
    assert "certified MOTION_FREE by this call" in text and "not a proof of infeasibility" in text and "never clamps the start or the goal" in text
    assert re.search(r"#define LOIKB_PLAN_SCRATCH_BYTES \(256ull << 20\)", _header())


def test_library_exports_every_plan_symbol():
    L = loik_amd.lib()
    decl = plan_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.PLAN_SYMBOLS), decl ^ set(capi.PLAN_SYMBOLS)
    assert len(capi.PLAN_SYMBOLS) == 2
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PATH_SYMBOLS,
                  capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS, capi.JACOBIAN_SYMBOLS, capi.COLLISION_SYMBOLS,
                  capi.MOTION_SYMBOLS, capi.AVOID_SYMBOLS, capi.SHORTCUT_SYMBOLS, capi.RETIME_SYMBOLS):
        assert not decl & set(older)


def test_version_and_struct_agree():
    L = loik_amd.lib()
    assert L.loikb_plan_version() == capi.PLAN_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_PLAN_VERSION 1\b", text)
    body = re.search(r"typedef struct loikb_plan_params \{(.*?)\} loikb_plan_params;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(double|int|unsigned long long)\s+([a-z_]+);", body, flags=re.M)
    assert [m[1] for m in members] == [f[0] for f in capi.PlanParams._fields_] == MEMBERS
    assert [m[0] for m in members] == ["double"] * 3 + ["unsigned long long"] + ["int"] * 4
    ctype = {"double": C.c_double, "int": C.c_int, "unsigned long long": C.c_ulonglong}
    assert [ctype[m[0]] for m in members] == [f[1] for f in capi.PlanParams._fields_]
    # three doubles, the seed, four ints: no padding anywhere
    assert C.sizeof(capi.PlanParams) == 48
    assert [getattr(capi.PlanParams, m).offset for m in MEMBERS] == [0, 8, 16, 24, 32, 36, 40, 44]
    names = re.search(r"enum \{(.*?)\};", text, flags=re.S).group(1)
    assert dict((k, int(v)) for k, v in re.findall(r"LOIKB_(PLAN_[A-Z_]+) = (\d+)", names)) == \
        {k: getattr(capi, k) for k in ("PLAN_FOUND", "PLAN_EXHAUSTED_ITERS", "PLAN_EXHAUSTED_NODES", "PLAN_START_BLOCKED", "PLAN_GOAL_BLOCKED",
                                       "PLAN_TOO_LONG", "PLAN_INVALID")}


def test_binding_and_mirror_have_the_methods():
    assert callable(getattr(loik_amd.BatchedLoik, "plan_paths"))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_plan.h"' in mirror
    for name in (r"PlanPaths\(", r"struct PlanResult\b"):
        assert re.search(r"\b%s" % name, mirror), name
    assert "loikb_plan_paths(" in mirror


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_retime_version() == capi.RETIME_ABI_VERSION == 1 and len(capi.RETIME_SYMBOLS) == 2
    assert L.loikb_shortcut_version() == capi.SHORTCUT_ABI_VERSION == 1 and len(capi.SHORTCUT_SYMBOLS) == 3
    assert L.loikb_motion_version() == capi.MOTION_ABI_VERSION == 1 and len(capi.MOTION_SYMBOLS) == 4
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_version() == capi.ABI_VERSION == 602
    for older in ("loik_amd_retime.h", "loik_amd_shortcut.h", "loik_amd_avoid.h", "loik_amd_motion.h", "loik_amd_collision.h", "loik_amd_multistart.h",
                  "loik_amd_path.h", "loik_amd_pose.h", "loik_amd_limits.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "loikb_plan_paths" not in text and "loikb_plan_version" not in text and "loik_amd_plan" not in text
