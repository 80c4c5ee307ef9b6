"""CPU: the gfx950 code of csrc/ics_img_mask.hip declares exactly its three kernels, uses no scratch memory and few enough registers
for eight workgroups of the cell kernel per CU (read from the AMDGPU metadata of the cross-compiled library like tests/test_isa.py and
tests/test_blur_width_isa.py: metadata only, no instruction is searched for), its LDS is the tile arithmetic DESIGN.md states ("Mask
choice on a resident frame"), and its tile and cell are those of the specification (tests/mask_ref.py)."""
import os
import re
import shutil
import subprocess

import mask_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024


def lds_table(tmp_path):
    """static LDS bytes per kernel of this unit (as tests/test_blur_width_isa.py reads them)"""
    from test_isa import LLVM
    work = tmp_path / "lds"
    work.mkdir()
    shutil.copy(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so"), work / "lib.so")
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=work, stdout=subprocess.DEVNULL)
    rows = {}
    for f in sorted(os.listdir(work)):
        if not f.endswith("gfx950"):
            continue
        pending = None
        for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=work, text=True).splitlines():
            m = re.match(r"    \.(group_segment_fixed_size|name):\s+(\S+)", line)
            if m and m.group(1) == "group_segment_fixed_size":
                pending = int(m.group(2))
            elif m and "k_img_mk_" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def test_mask_kernels_use_no_scratch_and_the_stated_lds(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_mask.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_mk_cells", "k_img_mk_pick", "k_img_mk_windows"]
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k in declared}
    assert sorted(found) == declared, sorted(found)
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    # a workgroup of the cell kernel is one wave per SIMD: the eight per CU the launcher starts need <= 512 / 8 registers
    assert found["k_img_mk_cells"]["vgpr_count"] <= 64, found["k_img_mk_cells"]
    # the tile and the cell of the specification, in the unit and in both headers
    d = {m: int(v) for m, v in re.findall(r"#define (MKT|MKLANES) (\d+)", src)}
    assert d == {"MKT": mr.TILE, "MKLANES": 256} and mr.TILE % mr.CELL == 0
    assert "#define MKCELL ICS_IMG_MASK_CELL" in src and "#define MKP (MKT + 1)" in src
    for header in (os.path.join(ROOT, "include", "ics_hip.h"), os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_kernels.h")):
        assert int(re.search(r"#define ICS_IMG_MASK_CELL (\d+)", open(header).read()).group(1)) == mr.CELL == 16
    # the staged luma is the tile and one more column and row, (MKT + 1)^2 floats, static; the pick kernel holds a score
    # and a candidate number per lane; the windows kernel has none
    cells_lds = 4 * (mr.TILE + 1) ** 2
    assert cells_lds == 16900
    lds = lds_table(tmp_path)
    assert lds == {"k_img_mk_cells": cells_lds, "k_img_mk_windows": 0, "k_img_mk_pick": 1024 * (8 + 4)}, lds
    assert "size_t ics_img_mask_lds() { return (size_t)MKP * MKP * sizeof(float); }" in src
    assert "`4 (MKT + 1)^2 = 16 900 B`" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert 8 * cells_lds <= LDS_PER_CU
    # the launcher: eight persistent workgroups per CU
    assert re.search(r"long grid = \(long\)\(cus > 0 \? cus : 256\) \* 8;", src)
