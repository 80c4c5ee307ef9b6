"""CPU: the gfx950 code of csrc/ics_img_psfest.hip declares exactly the kernels DESIGN.md names ("PSF from a frame pair on a resident
frame"), uses no scratch memory and spills nothing, its line kernels fit four waves a SIMD, and its LDS is what DESIGN.md states: the
line kernels take theirs at launch (two buffers of one line), the row kernel one float a lane beside it for the energy of its row, the
energy kernel 256 doubles; the transpose is the Wiener unit's kernel (read from the AMDGPU metadata of the cross-compiled library like
tests/test_wiener_isa.py: metadata only, no instruction is searched for)."""
import os
import re
import shutil
import subprocess

import wiener_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
LINE_KERNELS = ["k_img_pe_cols", "k_img_pe_crop", "k_img_pe_rows", "k_img_pe_solve"]
OTHER_KERNELS = ["k_img_pe_energy", "k_img_pe_tables"]
STATIC_LDS = {"k_img_pe_rows": 4096, "k_img_pe_energy": 2048}


def lds_table(tmp_path):
    """static LDS bytes per kernel of this unit (as tests/test_wiener_isa.py reads them: the size stands in front of the name)"""
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
            elif m and "k_img_pe_" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def test_psf_estimate_kernels_use_no_scratch_and_the_stated_lds(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_psfest.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("**PSF from a frame pair on a resident frame (`csrc/ics_img_psfest.hip`).**"):]
    section = section[:section.index("\n**", 10)] if "\n**" in section[10:] else section
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == sorted(LINE_KERNELS + OTHER_KERNELS)
    assert sorted(set(re.findall(r"`(k_img_pe_\w+)`", section))) == declared           # DESIGN.md names these and no other
    # the ISA tests of the Wiener and TV units collect their kernels by these over the whole library
    assert "k_img_wn_" not in src and "k_img_tvd_" not in src and "k_img_tvm_" not in src
    for own in ("ics_img_wiener.hip", "ics_img_tvdeconv.hip", "ics_img_tvmdeconv.hip"):   # ... and those units declare no kernel of this one
        assert "k_img_pe_" not in open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", own)).read()
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k in declared}
    assert sorted(found) == declared, sorted(found)
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    # a line's workgroup has up to 1024 lanes, 16 waves, four per SIMD: at most 512 / 4 registers
    for k in LINE_KERNELS:
        assert found[k]["vgpr_count"] <= 128, (k, found[k])
    # LDS: every line kernel takes 2 P float2 at launch; static are one float a lane of the row kernel (the row's share of the energy)
    # and 256 doubles of the energy kernel
    d = {m: int(v) for m, v in re.findall(r"#define (PE_LANES|PE_PLANES) (\d+)", src)}
    assert d == {"PE_LANES": 1024, "PE_PLANES": 6}
    lds = lds_table(tmp_path)
    assert lds == {k: STATIC_LDS.get(k, 0) for k in declared}, lds
    assert 4 * d["PE_LANES"] == STATIC_LDS["k_img_pe_rows"] and 8 * 256 == STATIC_LDS["k_img_pe_energy"]
    assert "`16 P` bytes" in section and "4 096 B" in section and "2 048 B" in section
    assert "ics_img_wiener_lds(Py)" in src and "ics_img_wiener_lds(ICS_IMG_WIENER_MAX)" in src        # the line kernels' launch-time LDS
    assert 16 * wr.MAX_SIDE + STATIC_LDS["k_img_pe_rows"] == 132 * 1024 <= LDS_PER_CU                  # the row kernel at 8192 points
    assert "getenv" not in src
