"""CPU: the joint-limits interface (include/loik_amd_limits.h) -- the header declares exactly its four entry points, the library
exports them, the binding's list and version match, and none of it leaks into the lists of the older headers."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_limits_version", "loikb_set_joint_limits", "loikb_update_ineq_constraints", "loikb_pose_get_limit_flags"}


def limits_symbols():
    text = open(os.path.join(ROOT, "include", "loik_amd_limits.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_the_four_entry_points():
    assert limits_symbols() == WANT


def test_library_exports_every_limits_symbol():
    L = loik_amd.lib()
    decl = limits_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.LIMITS_SYMBOLS), decl ^ set(capi.LIMITS_SYMBOLS)
    assert not decl & set(capi.EXPORTED_SYMBOLS)
    assert not decl & set(capi.POSE_SYMBOLS)


def test_versions_agree():
    L = loik_amd.lib()
    assert L.loikb_limits_version() == capi.LIMITS_ABI_VERSION == 1
    text = open(os.path.join(ROOT, "include", "loik_amd_limits.h")).read()
    assert re.search(r"#define LOIKB_LIMITS_VERSION 1\b", text)
    assert re.search(r"LOIKB_LIMIT_LOWER = %d, LOIKB_LIMIT_UPPER = %d\b" % (capi.LIMIT_LOWER, capi.LIMIT_UPPER), text)


def test_older_headers_and_lists_are_untouched():
    """the pose header and the base header keep their versions and their symbol counts (tests/test_pose_abi.py,
    tests/test_capi_abi.py pin them: this says why the limits live in a header of their own)"""
    L = loik_amd.lib()
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_version() == capi.ABI_VERSION == 602
