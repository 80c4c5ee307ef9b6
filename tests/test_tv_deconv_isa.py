"""CPU: the gfx950 code of csrc/ics_img_tvdeconv.hip declares exactly the kernels DESIGN.md names ("TV deconvolution on a resident
frame"), uses no scratch memory and spills nothing, its line kernels fit four waves a SIMD, and its LDS is what DESIGN.md states: the
line kernels take theirs at launch (two buffers of one line), the shrink pass static tiles of u and p; the tables, the transposes, the
rows of the PSF and the inverse rows are the Wiener unit's kernels, checked in tests/test_wiener_isa.py; the shrink pass serves the masked
unit too and is checked here (read from the AMDGPU metadata of the cross-compiled library like tests/test_wiener_isa.py: metadata only, no instruction is
searched for)."""
import os
import re

import wiener_ref as wr
from helpers import lds_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
LINE_KERNELS = ["k_img_tvd_cols", "k_img_tvd_n0", "k_img_tvd_psf_cols", "k_img_tvd_rows"]
OTHER_KERNELS = ["k_img_tvd_extend", "k_img_tvd_shrink"]
WIENER_LAUNCHES = ["ics_launch_img_wiener_tables", "ics_launch_img_wiener_transpose", "ics_launch_img_wiener_psf_rows", "ics_launch_img_wiener_inv_rows"]


def test_tv_deconvolve_kernels_use_no_scratch_and_the_stated_lds(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_tvdeconv.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("**TV deconvolution on a resident frame (`csrc/ics_img_tvdeconv.hip`).**"):]
    section = section[:section.index("\n**", 10)] if "\n**" in section[10:] else section
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == sorted(LINE_KERNELS + OTHER_KERNELS)
    assert sorted(set(re.findall(r"`(k_img_tvd_\w+)`", section))) == declared          # DESIGN.md names these and no other
    assert "k_img_wn_" not in src                                                      # tests/test_wiener_isa.py collects that unit's kernels by this
    for name in WIENER_LAUNCHES:                                                       # ... this unit launches them and redeclares none
        assert name + "(" in src and not re.search(r"\b(void|hipError_t)\s+" + name, src), name
    assert "k_img_tvd_psf_rows" not in src and "k_img_tvd_inv_rows" not in src
    assert re.search(r"\bvoid\s+ics_launch_img_tvd_shrink\(", src)                     # the one launcher of the shrink pass, the masked unit's too
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k.split("<")[0] in declared}
    assert sorted(set(k.split("<")[0] for k in found)) == declared, sorted(found)
    # the coupling, and the layout of u and z: planes (this unit) or the halves of a spectrum row (the masked unit)
    assert sorted(k for k in found if "<" in k) == ["k_img_tvd_shrink<%s, %s>" % (v, h) for v in ("false", "true") for h in ("false", "true")]
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    # a line's workgroup has up to 1024 lanes, 16 waves, four per SIMD: at most 512 / 4 registers
    for k in LINE_KERNELS:
        assert found[k]["vgpr_count"] <= 128, (k, found[k])
    # LDS: the shrink pass holds u on its 16 x 64 tile and one pixel around it and px, py on the
    # tile and one pixel above and left of it, three channels each; every line kernel takes 2 P float2 at launch and nothing static
    shared = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_wn_fft.h")).read()
    d = {m: int(v) for m, v in re.findall(r"#define (WN_LANES|TVD_TW|TVD_TH) (\d+)", shared + src)}
    assert d == {"WN_LANES": 1024, "TVD_TW": 64, "TVD_TH": 16}
    assert "_LANES 1024" not in src                                                    # the lanes of a line's workgroup are the shared header's
    shrink = 4 * 3 * (18 * 66 + 2 * 17 * 65)
    assert shrink == 40776
    lds = lds_table(tmp_path, "k_img_tvd_")
    assert sorted(lds) == sorted(found)
    for k, v in lds.items():                                                           # (the code object rounds the two arrays up to 16 bytes)
        want = (shrink + 15) // 16 * 16 if k.startswith("k_img_tvd_shrink") else 0
        assert v == want, (k, v)
    assert "`12 · (18 · 66 + 2 · 17 · 65) = 40 776 B`" in section and "`16 P` bytes" in section
    assert "ics_img_wiener_lds(Py)" in src and "ics_img_wiener_lds(WN_MAX)" in shared                 # the line kernels' launch-time LDS
    raised = re.search(r"wn_raise_lds<([^>]*)>\(Py, Px\)", src).group(1)                # ... its limit raised for every line kernel
    assert sorted(k.strip() for k in raised.split(",")) == LINE_KERNELS
    assert 16 * wr.MAX_SIDE == 128 * 1024 <= LDS_PER_CU
    assert "getenv" not in src
