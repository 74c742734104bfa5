"""CPU: the motion interface (include/loik_amd_motion.h) -- the header declares exactly its four entry points, the library exports them,
the binding's list, version, enum values and struct match, the mirror names them, none of it leaks into the older headers, and the
kernel behind the check keeps no static LDS."""
import os
import re

import loik_amd
from loik_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT = {"loikb_motion_version", "loikb_difference", "loikb_motion_clearance", "loikb_motion_clearance_path"}


def _header(name="loik_amd_motion.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def motion_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(loikb_[a-z_0-9]+)\s*\(", text))


def test_header_declares_exactly_its_entry_points():
    assert motion_symbols() == WANT
    assert re.search(r"typedef struct loikb_motion_params \{.*?\} loikb_motion_params;", _header(), flags=re.S)
    assert '#include "loik_amd_collision.h"' in _header()


def test_library_exports_every_motion_symbol():
    L = loik_amd.lib()
    decl = motion_symbols()
    for name in decl:
        assert hasattr(L, name), "libloik_amd.so does not export %s" % name
    assert decl == set(capi.MOTION_SYMBOLS), decl ^ set(capi.MOTION_SYMBOLS)
    assert len(capi.MOTION_SYMBOLS) == 4
    for older in (capi.EXPORTED_SYMBOLS, capi.POSE_SYMBOLS, capi.LIMITS_SYMBOLS, capi.TASKS_SYMBOLS, capi.MULTISTART_SYMBOLS, capi.PATH_SYMBOLS,
                  capi.TRACK_SYMBOLS, capi.ACCEL_SYMBOLS, capi.AXIS_SYMBOLS, capi.STEP_SYMBOLS, capi.JACOBIAN_SYMBOLS, capi.COLLISION_SYMBOLS):
        assert not decl & set(older)


def test_versions_enums_and_struct_agree():
    L = loik_amd.lib()
    assert L.loikb_motion_version() == capi.MOTION_ABI_VERSION == 1
    text = _header()
    assert re.search(r"#define LOIKB_MOTION_VERSION 1\b", text)
    assert re.search(r"LOIKB_MOTION_FREE = %d, LOIKB_MOTION_BLOCKED = %d, LOIKB_MOTION_UNDECIDED = %d, LOIKB_MOTION_INVALID = %d\b"
                     % (capi.MOTION_FREE, capi.MOTION_BLOCKED, capi.MOTION_UNDECIDED, capi.MOTION_INVALID), text)
    assert (capi.MOTION_FREE, capi.MOTION_BLOCKED, capi.MOTION_UNDECIDED, capi.MOTION_INVALID) == (0, 1, 2, 3)
    body = re.search(r"typedef struct loikb_motion_params \{(.*?)\} loikb_motion_params;", text, flags=re.S).group(1)
    members = re.findall(r"^\s*(double|int)\s+([a-z_]+);", body, flags=re.M)
    assert [m[1] for m in members] == [f[0] for f in capi.MotionParams._fields_] == ["margin", "tol", "max_evals", "flags"]
    assert [m[0] for m in members] == ["double", "double", "int", "int"]


def test_binding_and_mirror_have_the_methods():
    for name in ("difference", "motion_clearance", "path_clearance"):
        assert callable(getattr(loik_amd.BatchedLoik, name))
    mirror = open(os.path.join(ROOT, "include", "loik_amd", "loik.hpp")).read()
    assert '#include "../loik_amd_motion.h"' in mirror
    for name in ("Difference", "MotionClearance", "PathClearance"):
        assert re.search(r"\b%s\(" % name, mirror), name
    for sym in WANT - {"loikb_motion_version"}:
        assert sym + "(" in mirror, sym


def test_motion_check_kernels_have_no_static_lds():
    """both instantiations of k_motion_clearance in the library's gfx950 code object keep no LDS of their own (all of it is dynamic): the
    host's LDS-or-slab rule counts a kernel's static LDS against the 64 KB, and for the motion check that term must stay 0 for the rule
    to be fixed + aux > 65536 alone"""
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
                if name and "k_motion_clearance" in name.group(1):
                    found[name.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", rec).group(1))
    assert len(found) == 2 and {("ILb0E" in n, "ILb1E" in n) for n in found} == {(True, False), (False, True)}, sorted(found)
    for name, lds in found.items():
        assert lds == 0, (name, lds)


def test_older_headers_and_lists_are_untouched():
    L = loik_amd.lib()
    assert L.loikb_collision_version() == capi.COLLISION_ABI_VERSION == 1 and len(capi.COLLISION_SYMBOLS) == 9
    assert L.loikb_multistart_version() == capi.MULTISTART_ABI_VERSION == 1 and len(capi.MULTISTART_SYMBOLS) == 5
    assert L.loikb_jacobian_version() == capi.JACOBIAN_ABI_VERSION == 1 and len(capi.JACOBIAN_SYMBOLS) == 5
    assert L.loikb_version() == capi.ABI_VERSION == 602
    for older in ("loik_amd_collision.h", "loik_amd_multistart.h", "loik_amd_path.h", "loik_amd.h"):
        text = _header(older).lower()
        assert "loikb_motion" not in text and "loikb_difference" not in text and "loik_amd_motion" not in text
