"""CPU: the gfx950 code of csrc/ics_img_wavelet.hip uses no scratch memory (read from the AMDGPU metadata of the cross-compiled
library like tests/test_isa.py), and the fused kernel's registers and LDS tile leave room for the two workgroups of 512 lanes per CU
that DESIGN.md claims for it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wavelet_kernels_use_no_scratch_and_the_fused_one_fits_twice_into_a_cu(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_wavelet.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_wv_fused", "k_img_wv_scale"]
    tab = kernel_table(tmp_path)
    found = {}
    for name in declared:
        rows = {k: v for k, v in tab.items() if k == name or k.startswith(name + "<")}
        assert rows, "%s is not in the code object" % name
        found.update(rows)
        for k, v in rows.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    assert sorted(found) == ["k_img_wv_fused<false>", "k_img_wv_fused<true>", "k_img_wv_scale<false>", "k_img_wv_scale<true>"]
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    # the per-scale kernel keeps the 25 independent 12-byte loads of a lane in flight in registers (75 of them): its memory
    # parallelism comes from inside the lane, and DESIGN.md claims 4 waves per SIMD for it, 128 VGPRs
    for k in ("k_img_wv_scale<false>", "k_img_wv_scale<true>"):
        assert found[k]["vgpr_count"] <= 128, (k, found[k])
    # the fused kernel: two workgroups of 512 lanes = 16 waves per CU = 4 per SIMD, which 512 registers per lane and SIMD allow up to
    # 128 VGPRs; its LDS is dynamic (static part 0): 4 planes of the 76 x 60 staged tile, twice within 160 KB
    for k in ("k_img_wv_fused<false>", "k_img_wv_fused<true>"):
        assert found[k]["vgpr_count"] <= 128, (k, found[k])
        assert found[k].get("group_segment_fixed_size", 0) == 0, (k, found[k])
    tile = {m: int(v) for m, v in re.findall(r"#define (WVTW|WVTH|WVLANES) (\d+)", src)}
    fused = int(re.search(r"#define ICS_IMG_WAVELET_FUSED (\d+)", open(os.path.join(ROOT, "include", "ics_hip.h")).read()).group(1))
    halo = 2 * (2 ** fused - 1)
    lds = 4 * 4 * (tile["WVTW"] + 2 * halo) * (tile["WVTH"] + 2 * halo)
    assert tile == {"WVTW": 48, "WVTH": 32, "WVLANES": 512} and halo == 14 and lds == 72960
    assert 2 * lds <= 160 * 1024 < 3 * lds and 2 * tile["WVLANES"] <= 2048
