"""CPU: the multi-start interface (include/loik_amd_multistart.h) -- the header declares exactly its five entry points, the library
exports them, the binding's list and version match, and none of it leaks into the lists of the older headers."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_multistart_version", "loikb_multistart_set_ranges", "loikb_multistart_sample", "loikb_solve_pose_multistart",
        "loikb_multistart_get"}


def multistart_symbols():
    text = open(os.path.join(ROOT, "include", "loik_amd_multistart.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_the_five_entry_points():
    assert multistart_symbols() == WANT


def test_library_exports_every_multistart_symbol():
    L = loik_amd.lib()
    decl = multistart_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.MULTISTART_SYMBOLS), decl ^ set(capi.MULTISTART_SYMBOLS)
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS):
        assert not decl & set(older)


def test_versions_and_enums_agree():
    L = loik_amd.lib()
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1
    text = open(os.path.join(ROOT, "include", "loik_amd_multistart.h")).read()
    assert re.search(r"#define LOIKB_MULTISTART_VERSION 1\b", text)
    assert re.search(r"LOIKB_MS_PICK_NEAREST = %d, LOIKB_MS_PICK_FIRST = %d\b" % (capi.MS_PICK_NEAREST, capi.MS_PICK_FIRST), text)
    assert re.search(r"LOIKB_MS_GOAL_REACHED = %d, LOIKB_MS_GOAL_BEST_EFFORT = %d, LOIKB_MS_GOAL_FAILED = %d\b"
                     % (capi.MS_GOAL_REACHED, capi.MS_GOAL_BEST_EFFORT, capi.MS_GOAL_FAILED), text)
    fields = re.findall(r"\bLOIKB_MS_F_([A-Z_]+)", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert fields == ["WINNER", "GOAL_STATUS", "Q", "ERR", "COST", "NREACHED", "ROUND", "TIMING"]
    assert [getattr(capi, "MS_F_" + f) for f in fields] == list(range(8))
    assert capi.MS_PICKS == {"nearest": 0, "first": 1}


def test_params_struct_matches_the_header():
    """the field order of loikb_multistart_params, as the binding's ctypes struct has it"""
    text = open(os.path.join(ROOT, "include", "loik_amd_multistart.h")).read()
    body = re.search(r"typedef struct loikb_multistart_params \{(.*?)\} loikb_multistart_params;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [d.split()[-1] for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in capi.MultiStartParams._fields_] == ["seeds_per_goal", "rounds", "seed", "pick", "flags"]


def test_older_headers_and_lists_are_untouched():
    """the base, pose, limits and tasks headers keep their versions and their symbol counts (their own ABI tests pin them: this
    says why multi-start lives in a header of its own)"""
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_limits_version() == capi.LIMITS_ABI_VERSION == 1 and len(capi.LIMITS_SYMBOLS) == 4
    assert L.loikb_tasks_version() == capi.TASKS_ABI_VERSION == 1 and len(capi.TASKS_SYMBOLS) == 5
    for header in ("loik_amd.h", "loik_amd_pose.h", "loik_amd_limits.h", "loik_amd_tasks.h"):
        assert "multistart" not in open(os.path.join(ROOT, "include", header)).read()
