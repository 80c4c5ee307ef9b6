"""CPU: the gfx950 code of csrc/ics_img_tvmdeconv.hip declares exactly the kernels DESIGN.md names ("Masked TV deconvolution on a
resident frame"), uses no scratch memory and spills nothing, its line kernels fit four waves a SIMD, and its LDS is what DESIGN.md
states: the line kernels take theirs at launch (two buffers of one line), the setup and the count pass one word a lane; the tables, the transposes
and the rows of the PSF are the Wiener unit's kernels and the shrink pass, static tiles of u and p, the TV unit's, checked in
tests/test_wiener_isa.py and tests/test_tv_deconv_isa.py (read from the AMDGPU metadata of the
cross-compiled library like tests/test_tv_deconv_isa.py: metadata only, no instruction is searched for)."""
import os
import re

import wiener_ref as wr
from helpers import lds_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
LINE_KERNELS = ["k_img_tvm_blur_cols", "k_img_tvm_cols", "k_img_tvm_inv_rows", "k_img_tvm_psf_cols", "k_img_tvm_rows"]
OTHER_KERNELS = ["k_img_tvm_count", "k_img_tvm_setup"]
SHARED_LAUNCHES = ["ics_launch_img_wiener_tables", "ics_launch_img_wiener_transpose", "ics_launch_img_wiener_psf_rows", "ics_launch_img_tvd_shrink"]


def test_masked_tv_deconvolve_kernels_use_no_scratch_and_the_stated_lds(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_tvmdeconv.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("**Masked TV deconvolution on a resident frame (`csrc/ics_img_tvmdeconv.hip`).**"):]
    section = section[:section.index("\n**", 10)] if "\n**" in section[10:] else section
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == sorted(LINE_KERNELS + OTHER_KERNELS)
    assert sorted(set(re.findall(r"`(k_img_tvm_\w+)`", section))) == declared          # DESIGN.md names these and no other
    # tests/test_wiener_isa.py and tests/test_tv_deconv_isa.py collect their units' kernels by these
    assert "k_img_wn_" not in src and "k_img_tvd_" not in src
    for name in SHARED_LAUNCHES:                                                       # ... this unit launches them and redeclares none
        assert name + "(" in src and not re.search(r"\b(void|hipError_t)\s+" + name, src), name
    assert "k_img_tvm_psf_rows" not in src and "k_img_tvm_shrink" not in src
    for own in ("ics_img_tvdeconv.hip", "ics_img_wiener.hip"):                         # ... and those units declare no kernel of this one
        assert "k_img_tvm_" not in open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", own)).read()
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k.split("<")[0] in declared}
    assert sorted(set(k.split("<")[0] for k in found)) == declared, sorted(found)
    assert not [k for k in found if "<" in k]                                          # (the shrink pass, the one template, is the TV unit's)
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    # a line's workgroup has up to 1024 lanes, 16 waves, four per SIMD: at most 512 / 4 registers
    for k in LINE_KERNELS:
        assert found[k]["vgpr_count"] <= 128, (k, found[k])
    # LDS: the setup 256 ints and the count 256 64-bit sums; every line kernel takes 2 P float2 at launch and nothing static; the shrink
    # pass (the TV unit's kernel, its static tiles asserted in tests/test_tv_deconv_isa.py) is quoted in this section too
    shared = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_wn_fft.h")).read()
    d = {m: int(v) for m, v in re.findall(r"#define (WN_LANES|TVM_PER) (\d+)", shared + src)}
    assert d == {"WN_LANES": 1024, "TVM_PER": 8}
    assert "_LANES 1024" not in src and "TVM_TW" not in src and "TVM_TH" not in src    # the lanes are the shared header's, the tile the TV unit's
    assert d["WN_LANES"] * d["TVM_PER"] == wr.MAX_SIDE                                 # the column kernel holds a whole line in its lanes
    assert "static_assert(TVM_PER * WN_LANES == WN_MAX" in src
    shrink = 4 * 3 * (18 * 66 + 2 * 17 * 65)
    assert shrink == 40776
    lds = lds_table(tmp_path, "k_img_tvm_")
    assert sorted(lds) == sorted(found)
    for k, v in lds.items():
        assert v == {"k_img_tvm_setup": 1024, "k_img_tvm_count": 2048}.get(k, 0), (k, v)
    assert "`12 · (18 · 66 + 2 · 17 · 65) = 40 776 B`" in section and "`16 P` bytes" in section and "1 024 B" in section and "2 048 B" in section
    assert "ics_img_wiener_lds(Py)" in src and "ics_img_wiener_lds(WN_MAX)" in shared                 # the line kernels' launch-time LDS
    raised = re.search(r"wn_raise_lds<([^>]*)>\(Py, Px\)", src).group(1)                # ... its limit raised for every line kernel
    assert sorted(k.strip() for k in raised.split(",")) == LINE_KERNELS
    assert 16 * wr.MAX_SIDE == 128 * 1024 <= LDS_PER_CU
    assert "getenv" not in src
