"""CPU: the gfx950 code of csrc/ics_img_blurwidth.hip uses no scratch memory and at most 128 registers (read from the AMDGPU metadata
of the cross-compiled library like tests/test_isa.py and tests/test_noise_isa.py: metadata only, no instruction is searched for), its
LDS is the tile arithmetic DESIGN.md states ("Blur width on a resident frame") and fits a CU twice at the largest lag, and its tile is
the tile of the specification (tests/blur_width_ref.py)."""
import os
import re
import shutil
import subprocess

import blur_width_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024


def lds_table(tmp_path):
    """static LDS bytes per kernel of this unit (as tests/test_noise_isa.py reads them)"""
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
            elif m and "k_img_bw_" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def lds_bytes(d, L):
    """the x plane, ACTH rows at the pitch of the largest lag, ACTW + 128 + 1 lumas; the y plane, ACTH + L + 1 rows of
    ACTW; a sum per axis, lag and wave"""
    waves = d["ACTLANES"] // 64
    return 4 * (d["ACTH"] * (d["ACTW"] + br.MAX_LAG + 1) + (d["ACTH"] + L + 1) * d["ACTW"] + 2 * (L + 1) * waves)


def test_blur_width_kernels_use_no_scratch_and_fit_a_cu_twice_at_the_largest_lag(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_blurwidth.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_bw_partial", "k_img_bw_reduce"]
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k in declared}
    assert sorted(found) == declared, sorted(found)
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
        assert v["vgpr_count"] <= 128, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    d = {m: int(v) for m, v in re.findall(r"#define (ACTW|ACTH|ACTLANES|ACTCH) (\d+)", src)}
    assert d == {"ACTW": br.ACTW, "ACTH": br.ACTH, "ACTLANES": 256, "ACTCH": 8}
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    assert int(re.search(r"#define ICS_IMG_BLURWIDTH_MAX_LAG (\d+)", header).group(1)) == br.MAX_LAG == 128
    assert int(re.search(r"#define ICS_IMG_BLURWIDTH_MAX_LAG (\d+)", open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_kernels.h")).read()).group(1)) == 128
    # all of the partial kernel's LDS is dynamic, set by the launcher from this expression; the reduce kernel has none
    lds = lds_table(tmp_path)
    assert lds == {"k_img_bw_partial": 0, "k_img_bw_reduce": 0}, lds
    assert re.search(r"return \(\(size_t\)ACTH \* ACTSX \+ \(size_t\)\(ACTH \+ L \+ 1\) \* ACTW \+ \(size_t\)2 \* \(L \+ 1\) \* ACTWAVES\) \* sizeof\(float\);", src)
    assert "#define ACTWAVES (ACTLANES / 64)" in src and "#define ACTSX (ACTW + ICS_IMG_BLURWIDTH_MAX_LAG + 1)" in src
    assert lds_bytes(d, 128) == 70048 and lds_bytes(d, 64) == 51616 and lds_bytes(d, 16) == 37792     # the figures of DESIGN.md
    assert 2 * lds_bytes(d, br.MAX_LAG) <= LDS_PER_CU < 3 * lds_bytes(d, br.MAX_LAG)
    # the launcher: as many workgroups per CU as fit by LDS, four at most -- a workgroup is one wave per SIMD, so four need <= 128 registers
    assert re.search(r"int per_cu = \(int\)\(\(size_t\)160 \* 1024 / lds\);\s*per_cu = per_cu > 4 \? 4 : per_cu;", src)
    assert found["k_img_bw_partial"]["vgpr_count"] <= 512 // 4
