"""CPU: the voxel-world interface (include/loik_amd_grid.h) -- the header declares exactly its three entry points, the library exports
them, the binding's list, version and constants match, the mirror names the methods, the header says what it must about the bound, and
none of it leaks into the older headers and lists."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_grid_version", "loikb_collision_set_world_grid", "loikb_collision_get_world_grid"}


def _header(name="loik_amd_grid.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def grid_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert grid_symbols() == WANT
    assert '#include "loik_amd_collision.h"' in _header()
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    for phrase in ("g(0) = 0, g(d) = (2 |d| - 1)^2", "it is NOT a penetration depth", "lower bound of the distance", "at most sqrt(3) h",
                   "for whichever voxel i is read", "BLOCKED may be conservative by sqrt(3) h", "return LOIKB_ERR_STATE with a message that names the grid",
                   "On any error nothing of the handle changes", "then with a grid set the ns grid pairs in sphere order, then the self pairs",
                   "min_world includes the grid pairs", "bit for bit"):
        assert phrase in text, phrase


def test_library_exports_every_grid_symbol():
    L = loik_amd.lib()
    decl = grid_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.GRID_SYMBOLS) and len(capi.GRID_SYMBOLS) == 3
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.COLLISION_SYMBOLS, capi.MOTION_SYMBOLS, capi.AVOID_SYMBOLS, capi.SHORTCUT_SYMBOLS,
                  capi.RETIME_SYMBOLS, capi.PLAN_SYMBOLS, capi.BLEND_SYMBOLS):
        assert not decl & set(older)


def test_version_and_constants_agree():
    L = loik_amd.lib()
    assert L.loikb_grid_version() == capi.GRID_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_GRID_VERSION 1\b", text)
    assert re.search(r"#define LOIKB_CLR_WORLD_GRID %d\b" % capi.CLR_WORLD_GRID, text) and capi.CLR_WORLD_GRID == capi.CLR_SELF + 1 == 4
    assert re.search(r"#define LOIKB_GRID_MAX_DIM %d\b" % capi.GRID_MAX_DIM, text) and capi.GRID_MAX_DIM == 512
    assert re.search(r"#define LOIKB_GRID_MAX_VOXELS \(1u << 26\)", text) and capi.GRID_MAX_VOXELS == 1 << 26
    assert re.search(r"#define LOIKB_GRID_EMPTY 0xFFFFFFFFu", text) and capi.GRID_EMPTY == 0xFFFFFFFF
    # the kernels' copy of the largest value: three axes of 512 voxels
    assert 3 * (2 * 511 - 1) ** 2 < 0xF0000000


def test_binding_and_mirror_have_the_methods():
    for name in ("set_collision_grid", "collision_grid"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_grid.h"' in mirror
    for name in (r"SetCollisionGrid\(", r"GetCollisionGrid\(", r"ClearCollisionGrid\(", r"struct CollisionGrid\b"):
        assert re.search(r"\b%s" % name, mirror), name
    build = open(os.path.join(ROOT, "loik_amd", "_build.py")).read()
    assert "loik_amd_grid.h" in build and "loik_pose_grid.hpp" in build


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_collision_version() == capi.COLLISION_ABI_VERSION == 1 and L.loikb_motion_version() == capi.MOTION_ABI_VERSION == 1
    assert (capi.CLR_NONE, capi.CLR_WORLD_SPHERE, capi.CLR_WORLD_BOX, capi.CLR_SELF) == (0, 1, 2, 3)
    for older in ("loik_amd_blend.h", "loik_amd_plan.h", "loik_amd_retime.h", "loik_amd_shortcut.h", "loik_amd_avoid.h", "loik_amd_motion.h",
                  "loik_amd_collision.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "world_grid" not in text and "loik_amd_grid" not in text
