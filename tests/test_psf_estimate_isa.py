"""CPU: the gfx950 code of csrc/ics_img_psfest.hip declares exactly the kernels DESIGN.md names ("PSF from a frame pair on a resident
frame"), uses no scratch memory and spills nothing, its line kernels fit four waves a SIMD, and its LDS is what DESIGN.md states: the
line kernels take theirs at launch (two buffers of one line), the row kernel one float a lane beside it for the energy of its row, the
energy kernel 256 doubles; the transpose is the Wiener unit's kernel (read from the AMDGPU metadata of the cross-compiled library like
tests/test_wiener_isa.py: metadata only, no instruction is searched for)."""
import os
import re

import wiener_ref as wr
from helpers import lds_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
LINE_KERNELS = ["k_img_pe_cols", "k_img_pe_crop", "k_img_pe_rows", "k_img_pe_solve"]
OTHER_KERNELS = ["k_img_pe_energy", "k_img_pe_tables"]
STATIC_LDS = {"k_img_pe_rows": 4096, "k_img_pe_energy": 2048}


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
    shared = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_wn_fft.h")).read()
    d = {m: int(v) for m, v in re.findall(r"#define (WN_LANES|PE_PLANES) (\d+)", shared + src)}
    assert d == {"WN_LANES": 1024, "PE_PLANES": 6}
    assert "_LANES 1024" not in src                                                    # the lanes of a line's workgroup are the shared header's
    lds = lds_table(tmp_path, "k_img_pe_")
    assert lds == {k: STATIC_LDS.get(k, 0) for k in declared}, lds
    assert 4 * d["WN_LANES"] == STATIC_LDS["k_img_pe_rows"] and 8 * 256 == STATIC_LDS["k_img_pe_energy"]
    assert "`16 P` bytes" in section and "4 096 B" in section and "2 048 B" in section
    assert "ics_img_wiener_lds(Py)" in src and "ics_img_wiener_lds(WN_MAX)" in shared                 # the line kernels' launch-time LDS
    raised = re.search(r"wn_raise_lds<([^>]*)>\(Py, Px\)", src).group(1)                # ... its limit raised for every line kernel
    assert sorted(k.strip() for k in raised.split(",")) == LINE_KERNELS
    assert "ics_launch_img_wiener_transpose(" in src and not re.search(r"\bvoid\s+ics_launch_img_wiener_transpose", src)
    assert 16 * wr.MAX_SIDE + STATIC_LDS["k_img_pe_rows"] == 132 * 1024 <= LDS_PER_CU                  # the row kernel at 8192 points
    assert "getenv" not in src
