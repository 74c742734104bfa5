"""CPU: the avoidance interface (include/loik_amd_avoid.h) -- the header declares exactly its six entry points, the library exports them,
the binding's list, version, enum values and struct match, the mirror names them, none of it leaks into the older headers, and the
kernels behind it take no scratch and no static LDS."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_avoid_version", "loikb_clearance_gradient", "loikb_avoid_set", "loikb_avoid_get", "loikb_avoid_box", "loikb_avoid_get_result"}


def _header(name="loik_amd_avoid.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def avoid_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert avoid_symbols() == WANT
    assert re.search(r"typedef struct loikb_avoid_params \{.*?\} loikb_avoid_params;", _header(), flags=re.S)
    assert '#include "loik_amd_motion.h"' in _header()


def test_library_exports_every_avoid_symbol():
    L = loik_amd.lib()
    decl = avoid_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.AVOID_SYMBOLS), decl ^ set(capi.AVOID_SYMBOLS)
    assert len(capi.AVOID_SYMBOLS) == 6
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PATH_SYMBOLS,
                  capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS, capi.JACOBIAN_SYMBOLS, capi.COLLISION_SYMBOLS,
                  capi.MOTION_SYMBOLS):
        assert not decl & set(older)


def test_versions_enums_and_struct_agree():
    L = loik_amd.lib()
    assert L.loikb_avoid_version() == capi.AVOID_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_AVOID_VERSION 1\b", text)
    assert re.search(r"#define LOIKB_AVOID_MAX_SPHERES %d\b" % capi.AVOID_MAX_SPHERES, text)
    assert capi.AVOID_MAX_SPHERES >= 256
    assert re.search(r"LOIKB_AVOID_F_MIN_SEEN = %d,[^;]*LOIKB_AVOID_F_ACTIVE_STEPS,[^;]*LOIKB_AVOID_F_FLAGS \}" % capi.AVOID_F_MIN_SEEN, text, flags=re.S)
    assert (capi.AVOID_F_MIN_SEEN, capi.AVOID_F_ACTIVE_STEPS, capi.AVOID_F_FLAGS) == (0, 1, 2)
    body = re.search(r"typedef struct loikb_avoid_params \{(.*?)\} loikb_avoid_params;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(double|int)\s+([a-z_]+);", body, flags=re.M)
    assert [m[1] for m in members] == [f[0] for f in capi.AvoidParams._fields_] == ["d_safe", "d_influence", "kappa", "flags"]
    assert [m[0] for m in members] == ["double", "double", "double", "int"]


def test_binding_and_mirror_have_the_methods():
    for name in ("set_collision_avoidance", "clear_collision_avoidance", "clearance_gradient", "avoidance_box", "avoid_get"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_avoid.h"' in mirror
    for name in ("SetCollisionAvoidance", "ClearCollisionAvoidance", "ClearanceGradient", "AvoidanceBox"):
        assert re.search(r"\b%s\(" % name, mirror), name
    for sym in WANT - {"loikb_avoid_version"}:
        assert sym + "(" in mirror, sym


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_motion_version() == capi.MOTION_ABI_VERSION == 1 and len(capi.MOTION_SYMBOLS) == 4
    assert L.loikb_collision_version() == capi.COLLISION_ABI_VERSION == 1 and len(capi.COLLISION_SYMBOLS) == 9
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_version() == capi.ABI_VERSION == 602
    for older in ("loik_amd_motion.h", "loik_amd_collision.h", "loik_amd_multistart.h", "loik_amd_pose.h", "loik_amd_limits.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "loikb_avoid" not in text and "loikb_clearance_gradient" not in text and "loik_amd_avoid" not in text


def test_kernels_have_no_scratch_and_no_static_lds():
    """every instantiation of k_avoid_box in the library's gfx950 code object: no private segment (no spill, no runtime-indexed private
    array), no static LDS (the table is dynamic), eight instantiations (HBM x {gradient, query, step fp64, step fp32})"""
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import measure_clearance as MC
    llvm = MC.LLVM
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, capi._LIB_PATH, os.path.join(tmp, "copy.so")])
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)] + [len(blob)]
        for k in range(len(starts) - 1):
            part, co = os.path.join(tmp, "bundle%d" % k), os.path.join(tmp, "co%d" % k)
            open(part, "wb").write(blob[starts[k]:starts[k + 1]])
            subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                                   "--input=" + part, "--output=" + co])
            notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
            for rec in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", rec)
                if name and "k_avoid_box" in name.group(1):
                    found[name.group(1)] = tuple(int(re.search(r"\.%s:\s+(\d+)" % key, rec).group(1)) for key in ("group_segment_fixed_size", "private_segment_fixed_size"))
    assert len(found) == 8, sorted(found)
    for name, (lds, scratch) in found.items():
        assert lds == 0 and scratch == 0, (name, lds, scratch)
