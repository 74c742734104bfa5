"""CPU: the interface of include/loik_amd_gridnear.h -- the header declares exactly its entry points, the library exports them, the
binding's list, version and constant match, the mirror names the methods, the header says what it must, and none of it leaks into
loik_amd_grid.h, loik_amd_avoid.h and the older lists."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_gridnear_version", "loikb_collision_grid_set_nearest", "loikb_collision_grid_get_nearest", "loikb_grid_nearest_query"}


def _header(name="loik_amd_gridnear.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def gridnear_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert gridnear_symbols() == WANT
    assert '#include "loik_amd_grid.h"' in _header() and '#include "loik_amd_avoid.h"' in _header()
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    for phrase in ("the lowest linear index", "LOIKB_GRID_NO_VOXEL when no voxel is occupied", "bit for bit", "v <= true clearance <= d_u - r",
                   "Eight candidates do not guarantee the nearest cube", "Its clearance is v, the LOWER bound", "never farther",
                   "the partner loikb_avoid_box reports is nws + nwb", "d_safe plus up to sqrt(3) h", "a failed set leaves both as they were",
                   "it returns LOIKB_ERR_STATE while a grid is set and avoidance is latched", "On any error nothing of the handle changes",
                   "the lowest u on a tie", "the same bits"):
        assert phrase in text, phrase


def test_library_exports_every_symbol():
    L = loik_amd.lib()
    decl = gridnear_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.GRIDNEAR_SYMBOLS) and len(capi.GRIDNEAR_SYMBOLS) == len(WANT)
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.COLLISION_SYMBOLS, capi.MOTION_SYMBOLS, capi.AVOID_SYMBOLS, capi.SHORTCUT_SYMBOLS,
                  capi.RETIME_SYMBOLS, capi.PLAN_SYMBOLS, capi.BLEND_SYMBOLS, capi.GRID_SYMBOLS):
        assert not decl & set(older)


def test_version_and_constants_agree():
    L = loik_amd.lib()
    assert L.loikb_gridnear_version() == capi.GRIDNEAR_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_GRIDNEAR_VERSION 1\b", text)
    assert re.search(r"#define LOIKB_GRID_NO_VOXEL 0xFFFFFFFFu", text) and capi.GRID_NO_VOXEL == 0xFFFFFFFF


def test_binding_and_mirror_have_the_methods():
    for name in ("set_collision_grid_nearest", "collision_grid_nearest", "grid_nearest"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_gridnear.h"' in mirror
    for name in (r"SetCollisionGridNearest\(", r"GetCollisionGridNearest\(", r"GridNearest\(", r"struct GridNearestResult\b"):
        assert re.search(r"\b%s" % name, mirror), name
    build = open(os.path.join(ROOT, "loik_amd", "_build.py")).read()
    assert "loik_amd_gridnear.h" in build and "loik_pose_gridnear.hpp" in build


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_grid_version() == capi.GRID_ABI_VERSION == 1 and L.loikb_avoid_version() == capi.AVOID_ABI_VERSION == 1
    assert len(capi.GRID_SYMBOLS) == 3
    for older in ("loik_amd_grid.h", "loik_amd_avoid.h", "loik_amd_blend.h", "loik_amd_plan.h", "loik_amd_motion.h", "loik_amd_collision.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "gridnear" not in text and "grid_set_nearest" not in text and "no_voxel" not in text
    # the refusals of the grid header stay the default, and their messages now name the way out
    src = open(os.path.join(ROOT, "loik_amd", "csrc", "loik_host_pose.hpp")).read()
    assert src.count("(loikb_collision_grid_set_nearest) avoidance reads the grid") == 2
