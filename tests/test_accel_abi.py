"""CPU: the acceleration-limits interface (include/loik_amd_accel.h) -- the header declares exactly its four entry points, the
library exports them, the binding's list, version and enum values match, and none of it leaks into the lists of the older headers."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_accel_version", "loikb_set_joint_accel_limits", "loikb_accel_set_start_velocity", "loikb_accel_get_velocity"}


def _header(name="loik_amd_accel.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def accel_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_the_four_entry_points():
    assert accel_symbols() == WANT


def test_library_exports_every_accel_symbol():
    L = loik_amd.lib()
    decl = accel_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.ACCEL_SYMBOLS), decl ^ set(capi.ACCEL_SYMBOLS)
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS,
                  capi.PATH_SYMBOLS, capi.TRACK_SYMBOLS):
        assert not decl & set(older)


def test_versions_and_enums_agree():
    L = loik_amd.lib()
    assert L.loikb_accel_version() == capi.ACCEL_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_ACCEL_VERSION 1\b", text)
    assert re.search(r"LOIKB_LIMIT_ACCEL_LOWER = %d, LOIKB_LIMIT_ACCEL_UPPER = %d\b" % (capi.LIMIT_ACCEL_LOWER, capi.LIMIT_ACCEL_UPPER), text)
    assert (capi.LIMIT_ACCEL_LOWER, capi.LIMIT_ACCEL_UPPER) == (4, 8)
    # the four bits of the flag word are distinct, and INNER's new bit is beside the old ones
    assert len({capi.LIMIT_LOWER, capi.LIMIT_UPPER, capi.LIMIT_ACCEL_LOWER, capi.LIMIT_ACCEL_UPPER}) == 4
    assert capi.TRACK_IN_ACCEL == 8 and capi.TRACK_IN_LIMIT == 4
    assert re.search(r"8 = an acceleration limit did", _header("loik_amd_track.h"))


def test_binding_has_the_three_methods_and_a_table_entry():
    for name in ("set_joint_accel_limits", "set_start_velocity", "get_applied_velocity"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    assert capi.ACCEL_FIELD_DIMS == {"applied_velocity": ("nv",)} and "applied_velocity" not in capi.ACCEL_INT_FIELDS


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_pose_version() == capi.POSE_ABI_VERSION == 1 and len(capi.POSE_SYMBOLS) == 4
    assert L.loikb_limits_version() == capi.LIMITS_ABI_VERSION == 1 and len(capi.LIMITS_SYMBOLS) == 4
    assert L.loikb_track_version() == capi.TRACK_ABI_VERSION == 1 and len(capi.TRACK_SYMBOLS) == 3
    assert L.loikb_version() == capi.ABI_VERSION == 602
