"""CPU: the gfx950 code of csrc/ics_img_tvdenoise.hip uses no scratch memory (read from the AMDGPU metadata of the cross-compiled
library like tests/test_isa.py), and the blocked kernel's registers leave room for the two workgroups per CU its LDS tile allows."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tv_denoise_kernels_use_no_scratch(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_tvdenoise.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_tv_block", "k_img_tv_final", "k_img_tv_iter"]
    tab = kernel_table(tmp_path)
    found = {}
    for name in declared:
        rows = {k: v for k, v in tab.items() if k == name or k.startswith(name + "<")}
        assert rows, "%s is not in the code object" % name
        found.update(rows)
        for k, v in rows.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert v["vgpr_count"] <= 64, (k, v)       # 8 waves per SIMD as far as registers go: LDS and memory set the pace
    assert sorted(found) == ["k_img_tv_block<false>", "k_img_tv_block<true>", "k_img_tv_final", "k_img_tv_iter<false>", "k_img_tv_iter<true>"]
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
