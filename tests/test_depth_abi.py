"""CPU: the interface of include/loik_amd_depth.h -- the header declares exactly its entry points, the library exports them, the
binding's list, version and constants match, the mirror names the methods, the header says what it must, and none of it leaks into
loik_amd_grid.h, loik_amd_gridnear.h and the older lists."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_depth_version", "loikb_collision_grid_integrate_depth", "loikb_collision_grid_integrate_points", "loikb_collision_grid_get_occupancy"}


def _header(name="loik_amd_depth.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def depth_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert depth_symbols() == WANT
    assert '#include "loik_amd_gridnear.h"' in _header()
    text = " ".join(re.sub(r"\n \*", " ", _header()).split())
    for phrase in ("one point one voxel", "would miss anything thinner than a voxel", "certifies nothing", "The points win over the carve",
                   "The filter wins over the points", "band >= (sqrt(3) / 2) h a cleared voxel lies wholly in front of the measured surface",
                   "filter_pad must cover (sqrt(3) / 2) h plus the sensor's noise", "A pixel without a return carves nothing",
                   "a point exactly on the low face is in, one exactly on the high face is out", "else LOIKB_ERR_STATE",
                   "Everything is validated before anything changes", "on any error nothing of the handle changes",
                   "a call at sensor rate allocates nothing after the first of its size", "for whichever call set the grid",
                   "returns the bits it returned before this header existed", "Out of scope: log-odds or TSDF weights"):
        assert phrase in text, phrase


def test_library_exports_every_symbol():
    L = loik_amd.lib()
    decl = depth_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.DEPTH_SYMBOLS) and len(capi.DEPTH_SYMBOLS) == len(WANT)
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.COLLISION_SYMBOLS, capi.MOTION_SYMBOLS, capi.AVOID_SYMBOLS, capi.SHORTCUT_SYMBOLS,
                  capi.RETIME_SYMBOLS, capi.PLAN_SYMBOLS, capi.BLEND_SYMBOLS, capi.GRID_SYMBOLS, capi.GRIDNEAR_SYMBOLS):
        assert not decl & set(older)


def test_version_and_constants_agree():
    L = loik_amd.lib()
    assert L.loikb_depth_version() == capi.DEPTH_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_DEPTH_VERSION 1\b", text)
    for name, value in (("F32", capi.DEPTH_F32), ("U16", capi.DEPTH_U16), ("REPLACE", capi.DEPTH_REPLACE), ("FUSE", capi.DEPTH_FUSE),
                        ("Q_DEVICE", capi.DEPTH_Q_DEVICE), ("MAX_IMAGE", capi.DEPTH_MAX_IMAGE), ("MAX_FILTER", capi.DEPTH_MAX_FILTER)):
        assert re.search(r"#define LOIKB_DEPTH_%s %d\b" % (name, value), text), name
    assert capi.DEPTH_Q_DEVICE & capi.IN_DEVICE == 0
    # the structs of the binding are the header's, field for field
    for struct, cls in (("loikb_depth_camera", capi.DepthCamera), ("loikb_depth_params", capi.DepthParams)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
        names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def test_binding_and_mirror_have_the_methods():
    for name in ("integrate_depth", "integrate_points", "collision_occupancy"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_depth.h"' in mirror
    for name in (r"IntegrateDepth\(", r"IntegratePoints\(", r"GetCollisionOccupancy\(", r"struct DepthCamera\b", r"struct DepthStats\b"):
        assert re.search(r"\b%s" % name, mirror), name
    build = open(os.path.join(ROOT, "loik_amd", "_build.py")).read()
    assert "loik_amd_depth.h" in build and "loik_pose_depth.hpp" in build


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_version() == capi.ABI_VERSION == 602
    assert L.loikb_grid_version() == capi.GRID_ABI_VERSION == 1 and L.loikb_gridnear_version() == capi.GRIDNEAR_ABI_VERSION == 1
    assert len(capi.GRID_SYMBOLS) == 3 and len(capi.GRIDNEAR_SYMBOLS) == 4
    for older in ("loik_amd_grid.h", "loik_amd_gridnear.h", "loik_amd_avoid.h", "loik_amd_blend.h", "loik_amd_plan.h", "loik_amd_motion.h",
                  "loik_amd_collision.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "loikb_depth" not in text and "loik_amd_depth" not in text and "integrate_points" not in text and "get_occupancy" not in text, older
    # one build for every call that sets a grid: the tail of loikb_collision_set_world_grid is a helper, not a copy
    src = open(os.path.join(ROOT, "loik_amd", "csrc", "loik_host_pose.hpp")).read()
    assert src.count("hipLaunchKernelGGL(k_grid_x,") == 1 and src.count("grid_build_swap(S, ") == 2
    assert src.count("(loikb_collision_grid_set_nearest) avoidance reads the grid") == 2
