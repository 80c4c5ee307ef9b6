"""CPU: the gfx950 code of csrc/ics_img_edges.hip declares exactly the kernels DESIGN.md names ("Edge prediction and fast blind PSF on a
resident frame"), uses no scratch memory and spills nothing, its registers leave room for the workgroups per CU its launchers assume,
and its LDS is what DESIGN.md states: the blocked shock kernel and the three counting kernels of the select take theirs at launch (8
planes of 48 x 48 floats; 2048 bins of 4 B per population), static are the twelve prefixes of a counting kernel, the four wave sums
of the select and the masked row kernel's float a lane (read from the AMDGPU metadata of the cross-compiled library like tests/test_psf_estimate_isa.py: metadata only, no
instruction is searched for)."""
import os
import re

import edges_ref as er
from helpers import lds_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
TEMPLATES = ["k_img_ed_hist", "k_img_ed_keys", "k_img_ed_mask", "k_img_ed_mask_keys", "k_img_ed_recompute", "k_img_ed_shock", "k_img_ed_shock_block"]
PLAIN = ["k_img_ed_rows", "k_img_ed_select"]
COUNTING = ["k_img_ed_hist", "k_img_ed_keys", "k_img_ed_recompute"]


def test_edge_kernels_use_no_scratch_and_the_stated_lds(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_edges.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("**Edge prediction and fast blind PSF on a resident frame (`csrc/ics_img_edges.hip`).**"):]
    section = section[:section.index("\n**", 10)] if "\n**" in section[10:] else section
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == sorted(TEMPLATES + PLAIN)
    assert sorted(set(re.findall(r"`(k_img_ed_\w+)`", section))) == declared           # DESIGN.md names these and no other
    # the ISA tests of other units collect their kernels by these prefixes over the whole library
    assert all(k.startswith("k_img_ed_") for k in declared)
    tab = kernel_table(tmp_path)
    want = sorted([k + v for k in TEMPLATES for v in ("<false>", "<true>")] + PLAIN)
    found = {k: v for k, v in tab.items() if k.split("<")[0] in declared}
    assert sorted(found) == want, sorted(found)
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    d = {m: int(v) for m, v in re.findall(r"#define (EDB|EDSL|EDB0|EDB1|EDLANES|EDPOP|EDHK) (\d+)", src)}
    assert d == {"EDB": 32, "EDSL": 512, "EDB0": 11, "EDB1": 10, "EDLANES": 256, "EDPOP": 12, "EDHK": 4} and d["EDB0"] + 2 * d["EDB1"] == 31
    assert "#define EDT ICS_IMG_SHOCK_BLOCK" in src and er.SHOCK_BLOCK == 4
    assert re.search(r"#define ICS_IMG_SHOCK_BLOCK 4\b", open(os.path.join(ROOT, "include", "ics_hip.h")).read())
    # static LDS: the prefixes of a counting kernel, the wave sums of the select; everything else is taken at launch
    lds = lds_table(tmp_path, "k_img_ed_")
    static = {k: (4 * d["EDPOP"] if k.split("<")[0] in COUNTING else 4 * d["EDLANES"] // 64 if k == "k_img_ed_select" else 0) for k in want}
    static["k_img_ed_rows"] = 4 * 1024                  # the masked row kernel: one float a lane for the energy of its row, as k_img_pe_rows
    assert lds == static, lds
    # ... its line of up to 8192 points is taken at launch like the pair solve's, its limit raised the same way; a line's workgroup has up to
    # 1024 lanes, four waves per SIMD: at most 128 registers
    shared = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_wn_fft.h")).read()
    assert "#define WN_LANES 1024" in shared and "__launch_bounds__(WN_LANES) void k_img_ed_rows" in src and "wn_raise_lds<k_img_ed_rows>(Py, Px)" in src
    assert found["k_img_ed_rows"]["vgpr_count"] <= 128, found["k_img_ed_rows"]
    assert 16 * 8192 + static["k_img_ed_rows"] <= LDS_PER_CU and "4 096 B" in section
    # the blocked shock route: 8 planes of (32 + 4 EDT)^2 floats, two workgroups of 512 lanes per CU = 4 waves per SIMD: 128 registers
    side = d["EDB"] + 4 * er.SHOCK_BLOCK
    tile = 8 * 4 * side * side
    assert side == 48 and tile == 73728 and 2 * tile <= LDS_PER_CU < 3 * tile
    assert re.search(r"size_t ics_img_shock_block_lds\(\) \{ return \(size_t\)8 \* EDN \* sizeof\(float\); \}", src)
    assert "73 728 B" in section
    for v in ("<false>", "<true>"):
        assert found["k_img_ed_shock_block" + v]["vgpr_count"] <= 128, found["k_img_ed_shock_block" + v]
    # the select's histograms: 2048 bins x 4 B per population, 4 populations "vector", 12 "channel"; the launcher's workgroups per CU
    hist = {True: 4 * 2 ** d["EDB0"] * 4, False: 12 * 2 ** d["EDB0"] * 4}
    assert hist == {True: 32768, False: 98304} and "32 768 B" in section and "98 304 B" in section
    assert re.search(r"return \(size_t\)\(coupling \? 4 : 12\) \* EDBINS \* sizeof\(unsigned\);", src)
    m = re.search(r"const int per_cu = coupling \? (\d) : (\d);", src)
    per_cu = {True: int(m.group(1)), False: int(m.group(2))}
    assert per_cu == {True: 4, False: 1}
    for vec, name in ((False, "<false>"), (True, "<true>")):
        assert per_cu[vec] * (hist[vec] + 4 * d["EDPOP"]) <= LDS_PER_CU and 2 * hist[False] > LDS_PER_CU   # "channel" fits once
        for k in COUNTING:      # a workgroup of 256 lanes is one wave per SIMD: w workgroups per CU leave each 512 / w registers
            assert found[k + name]["vgpr_count"] <= 512 // per_cu[vec] and found[k + name]["vgpr_count"] <= 128, (k + name, found[k + name])
        for k in ("k_img_ed_mask", "k_img_ed_mask_keys"):
            assert found[k + name]["vgpr_count"] <= 64, (k + name, found[k + name])    # eight workgroups per CU
        # (k_img_ed_shock, a lane per pixel with 45 pixel loads in flight, has no LDS and its launcher assumes no occupancy)
    assert "getenv" not in src
