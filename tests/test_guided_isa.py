"""CPU: the gfx950 code of csrc/ics_img_guided.hip uses no scratch memory (read from the AMDGPU metadata of the cross-compiled
library like tests/test_isa.py), and its registers and LDS tiles leave the occupancy DESIGN.md ("Guided filter") claims: 64 VGPRs
or fewer, so the 8 waves per SIMD the hardware allows and LDS alone decides how many workgroups of 256 lanes share a CU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lds_bytes(r, C, K):
    """csrc/ics_img_guided.hip gf_coef_lds: 3 planes of I' with an r halo around the C x C region, one scratch plane, K planes of sums"""
    return 4 * (3 * (C + 2 * r) * (C + 2 * r + 1) + (C + 2 * r) * (C + 1) + K * C * (C + 1))


def test_guided_kernels_use_no_scratch_and_their_tiles_fit_the_lds(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_guided.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_gf_apply", "k_img_gf_coef", "k_img_gf_fused"]
    tab = kernel_table(tmp_path)
    found = {}
    for name in declared:
        rows = {k: v for k, v in tab.items() if k == name or k.startswith(name + "<")}
        assert rows, "%s is not in the code object" % name
        found.update(rows)
        for k, v in rows.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    assert sorted(found) == ["k_img_gf_apply<false>", "k_img_gf_apply<true>", "k_img_gf_coef<false>", "k_img_gf_coef<true>",
                             "k_img_gf_fused<false>", "k_img_gf_fused<true>"]
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    for k, v in found.items():
        assert v["vgpr_count"] <= 64, (k, v)                              # 8 waves per SIMD: registers never limit the occupancy
        assert v.get("group_segment_fixed_size", 0) == 0, (k, v)         # the LDS is dynamic, sized by the radius
    tile = {m: int(v) for m, v in re.findall(r"#define (GFT|GFP|GFLANES) (\d+)", src)}
    assert tile == {"GFT": 32, "GFP": 4, "GFLANES": 256} and tile["GFT"] // tile["GFP"] * tile["GFT"] == tile["GFLANES"]
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    rmax = int(re.search(r"#define ICS_IMG_GUIDED_MAX_RADIUS (\d+)", header).group(1))
    fused = int(re.search(r"#define ICS_IMG_GUIDED_FUSED_RADIUS (\d+)", header).group(1))
    lds = 160 * 1024
    region = lambda r: (32 + 2 * r + 3) // 4 * 4                          # noqa: E731  the fused coefficient region: whole groups of GFP
    # route 1 fits at the largest radius; the fused tile at FUSED_RADIUS and not one above; workgroups per CU at r = 4, 8
    assert (rmax, fused) == (32, 8)
    assert lds_bytes(rmax, 32, 9) == 162432 <= lds and lds_bytes(rmax, 32, 6) == 149760
    assert lds_bytes(fused, region(fused), 9) == 147136 <= lds < lds_bytes(fused + 1, region(fused + 1), 9) == 173696
    assert [lds // lds_bytes(r, 32, 9) for r in (4, 8, 16, 32)] == [2, 2, 1, 1]
    assert [lds // lds_bytes(r, 32, 6) for r in (4, 8, 16, 32)] == [3, 2, 1, 1]
    assert [lds // lds_bytes(r, region(r), K) for r, K in ((4, 6), (4, 9), (8, 6), (8, 9))] == [2, 1, 1, 1]
