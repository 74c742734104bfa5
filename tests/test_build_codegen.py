"""The flat iteration kernels' code generation (loik_amd/_build.py::FLAT_FLAGS, loik_amd/csrc/loik_flat_inst.hpp): k_flat2 / k_flat1 live in a
code object of their own whose LDS accesses are single 64-bit instructions -- a ds_read2_b64 occupies the LDS pipe 3.4 x as long as a
ds_read_b64 on MI355X (scripts/ubench/lds_rate.hip).  A toolchain or flag change that silently brought the merged forms back would cost the
whole body ~10 % and the headline ~4 % without failing any parity test: this looks at the shipped library.  CPU only (llvm-objdump)."""
import os
import shutil
import subprocess
import tempfile

import pytest

from loik_amd import _build

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="no llvm-objdump in this image")
def test_flat_kernels_have_their_own_code_object_without_merged_lds_accesses():
    lib = _build.build()
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "lib.so")
        shutil.copy(lib, tmp)
        subprocess.run([OBJDUMP, "--offloading", tmp], check=True, capture_output=True)
        objs = sorted(f for f in os.listdir(d) if "amdgcn" in f and "gfx950" in f)
        assert len(objs) == 2, objs   # (host unit, flat unit)
        seen = {}
        for f in objs:
            dis = subprocess.run([OBJDUMP, "-d", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
            flat = dis.count("k_flat2") + dis.count("k_flat1") > 0
            seen[flat] = {op: dis.count(op + " ") for op in ("ds_read2_b64", "ds_read2st64_b64", "ds_write2_b64", "ds_read_b64", "ds_write_b64")}
        assert set(seen) == {True, False}, seen          # the flat kernels are in one object only
        fl, host = seen[True], seen[False]
        # a few merged reads remain outside the loops (explicit two-word loads of the load path); the loops' thousands are single accesses
        assert fl["ds_read_b64"] > 20 * (fl["ds_read2_b64"] + fl["ds_read2st64_b64"]) and fl["ds_write2_b64"] == 0, fl
        assert host["ds_read2_b64"] > 100, host           # (and the other kernels keep the default code generation)


def test_flat_flags_are_what_the_design_says():
    assert "-load-store-opt" in _build.FLAT_FLAGS and "-amdgpu-load-store-vectorizer=0" in _build.FLAT_FLAGS
    assert "loik_flat_kernels.hip" in _build.SOURCES


READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.mark.skipif(not os.path.exists(READELF), reason="no llvm-readelf in this image")
def test_flat_kernels_have_no_static_lds():
    """k_flat2 / k_flat1 address their gathers by ABSOLUTE LDS address (loik_flat2.hpp::lds_abs): their dynamic LDS must start at LDS
    address 0, i.e. the kernels must own no static LDS (`.group_segment_fixed_size: 0` in the code object's notes).  The kernels check the
    same at run time (FLAT_COUNTERS_ERR bit 2); this is the build-time half."""
    import re
    import struct
    data = open(_build.build(), "rb").read()
    found, idx = 0, 0
    with tempfile.TemporaryDirectory() as d:
        while True:
            i = data.find(b"\x7fELF\x02\x01\x01\x40", idx)   # ELFCLASS64, little endian, OSABI = AMDGPU_HSA
            if i < 0:
                break
            shoff = struct.unpack_from("<Q", data, i + 0x28)[0]
            shentsize, shnum = struct.unpack_from("<HH", data, i + 0x3A)
            path = os.path.join(d, "co.elf")
            with open(path, "wb") as f:
                f.write(data[i:i + shoff + shentsize * shnum])
            notes = subprocess.run([READELF, "--notes", path], check=True, capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "k_flat2" in name or "k_flat1" in name:
                    assert re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1) == "0", name
                    found += 1
            idx = i + 8
    assert found >= 20, found


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) or os.environ.get("LOIKB_SKIP_CODEGEN_GUARD") == "1", reason="no hipcc / switched off")
def test_flat_kernels_iteration_loops_hold_no_more_scratch_reloads_than_known():
    """The flat unit compiled to assembly with the shipped flags (one minute), the iteration loop of the kernels the benchmarks run found by the
    compiler's own loop annotations (scripts/r05/loopstat.py), its scratch loads counted.  Since the unit is scheduled by the iterative ILP scheduler the
    register allocation sits near a tipping point: twice in round 6 a small change of the source moved reloads INTO the loop (13 -> 43: whole body +16 %,
    -> 123: 5 x slower) with every parity test green.  The 11-13 that are there belong to the block of the full stopping logic, which a quiet iteration
    never enters; a number above the bound means: look at the loop before measuring anything (tests/test_engines.py holds the run-time half)."""
    import re
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "flat.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=on", "-std=c++17", "-fPIC", "-I", os.path.join(root, "include"), "-DLOIKB_FLAT_SEPARATE_TU",
               "-x", "hip", os.path.join(root, "loik_amd", "csrc", "loik_flat_kernels.hip"), "-S", "--cuda-device-only", "-o", asm] + list(_build.FLAT_FLAGS)
        subprocess.run(cmd, check=True, capture_output=True)
        # (mangled template arguments: k_flat2<NA 10, SLICED, HM 0, LOG 0, MUR>, k_flat1<NA 10, SLICED, HM 0, LOG 0, MUR 0>)
        kernels = {"k_flat2ILi10ELb1ELi0ELb0ELi2E": "headline: time-sliced, lazily populated table", "k_flat2ILi10ELb0ELi0ELb0ELi0E": "ordered / small batches",
                   "k_flat2ILi10ELb1ELi0ELb0ELi0E": "time-sliced, full table", "k_flat1ILi10ELb1ELi0ELb0ELi0E": "whole body, time-sliced",
                   "k_flat1ILi10ELb0ELi0ELb0ELi0E": "whole body, ordered"}
        for key, what in kernels.items():
            out = subprocess.run([sys.executable, os.path.join(root, "scripts", "r05", "loopstat.py"), asm, key], check=True, capture_output=True, text=True).stdout
            line = out.strip().splitlines()[-1]
            loads = sum(int(n) for n in re.findall(r"scratch_load_\w+ (\d+)", line))
            assert "loop header" in line, line
            assert loads <= 20, "%s (%s): %d scratch loads in the iteration loop -- %s" % (key, what, loads, line)
