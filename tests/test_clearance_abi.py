"""CPU: the collision interface (include/loik_amd_collision.h) -- the header declares exactly its nine entry points, the library exports
them, the binding's list, version, enum values and struct match, the mirrors name them, and none of it leaks into the older headers."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_collision_version", "loikb_collision_set_spheres", "loikb_collision_set_world", "loikb_collision_set_self_pairs",
        "loikb_collision_num_self_pairs", "loikb_clearance", "loikb_clearance_set_multistart", "loikb_clearance_get_multistart",
        "loikb_clearance_get_multistart_result"}


def _header(name="loik_amd_collision.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def collision_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert collision_symbols() == WANT
    # ... and the one type they take
    assert re.search(r"typedef struct loikb_clearance_params \{.*?\} loikb_clearance_params;", _header(), flags=re.S)


def test_library_exports_every_collision_symbol():
    L = loik_amd.lib()
    decl = collision_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.COLLISION_SYMBOLS), decl ^ set(capi.COLLISION_SYMBOLS)
    assert len(capi.COLLISION_SYMBOLS) == 9
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS,
                  capi.PATH_SYMBOLS, capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS, capi.JACOBIAN_SYMBOLS):
        assert not decl & set(older)


def test_versions_and_enums_agree():
    L = loik_amd.lib()
    assert L.loikb_collision_version() == capi.COLLISION_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_COLLISION_VERSION 1\b", text)
    assert re.search(r"#define LOIKB_CLR_MAX_SPHERES %d\b" % capi.CLR_MAX_SPHERES, text)
    assert re.search(r"LOIKB_CLR_NONE = %d, LOIKB_CLR_WORLD_SPHERE = %d, LOIKB_CLR_WORLD_BOX = %d, LOIKB_CLR_SELF = %d\b"
                     % (capi.CLR_NONE, capi.CLR_WORLD_SPHERE, capi.CLR_WORLD_BOX, capi.CLR_SELF), text)
    assert (capi.CLR_NONE, capi.CLR_WORLD_SPHERE, capi.CLR_WORLD_BOX, capi.CLR_SELF) == (0, 1, 2, 3)
    assert re.search(r"LOIKB_MS_GOAL_IN_COLLISION = %d\b" % capi.MS_GOAL_IN_COLLISION, text) and capi.MS_GOAL_IN_COLLISION == 8
    # the result fields count from 0 in the header's order
    fields = re.search(r"enum \{ (LOIKB_CLR_MS_F_CLEARANCE = 0,.*?LOIKB_CLR_MS_F_INSTANCE) \};", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"LOIKB_CLR_MS_F_([A-Z]+)", fields) == ["CLEARANCE", "WITNESS", "NCLEAR", "INSTANCE"]
    assert (capi.CLR_MS_F_CLEARANCE, capi.CLR_MS_F_WITNESS, capi.CLR_MS_F_NCLEAR, capi.CLR_MS_F_INSTANCE) == (0, 1, 2, 3)
    # the struct of the binding has the header's members in the header's order
    members = re.findall(r"^\s*(?:double|int)\s+([a-z_]+);",
                         re.search(r"typedef struct loikb_clearance_params \{(.*?)\} loikb_clearance_params;", text, flags=re.S).group(1), flags=re.M)
    assert members == [f[0] for f in capi.ClearanceParams._fields_] == ["margin", "flags"]


def test_binding_and_mirror_have_the_methods():
    for name in ("set_collision_spheres", "set_collision_world", "set_self_collision", "num_self_pairs", "clearance",
                 "set_multistart_clearance", "clear_multistart_clearance", "multistart_clearance", "multistart_clearance_get"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    import inspect
    assert "clearance_margin" in inspect.signature(loik_amd.BatchedLoik.SolvePoseMultiStart).parameters
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_collision.h"' in mirror
    for name in ("setCollisionSpheres", "setCollisionWorld", "setSelfCollision", "NumSelfPairs", "Clearance", "setMultiStartClearance",
                 "clearMultiStartClearance", "MultiStartClearance"):
        assert re.search(r"\b%s\(" % name, mirror), name
    for sym in WANT - {"loikb_collision_version"}:
        assert sym + "(" in mirror, sym


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_jacobian_version() == capi.JACOBIAN_ABI_VERSION == 1 and len(capi.JACOBIAN_SYMBOLS) == 5
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert (capi.MS_GOAL_REACHED, capi.MS_GOAL_BEST_EFFORT, capi.MS_GOAL_FAILED) == (1, 2, 4)
    # the multi-start header says nothing of the new class: it is this header's
    assert "collision" not in _header("loik_amd_multistart.h").lower() and "clearance" not in _header("loik_amd_multistart.h").lower()
