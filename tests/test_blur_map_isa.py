"""CPU: the gfx950 code of csrc/ics_img_blurmap.hip uses no scratch memory and spills nothing (read from the AMDGPU metadata of the
cross-compiled library like tests/test_blur_width_isa.py: metadata only, no instruction is searched for), its LDS is the tile
arithmetic DESIGN.md states ("Blur map on a resident frame") and fits a CU twice at the largest radius, and its register count allows
the two workgroups of 512 lanes per CU that the launcher asks for."""
import os
import re
import shutil
import subprocess

import blur_map_ref as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
RADII = list(range(2, bm.MAX_RADIUS + 1))


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
            elif m and "k_img_bm" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def lds_bytes(d, r):
    """the luma with its halo of r + 2; Sh of both sigmas on its rows and the tile's columns + 4; S of both on the tile + 4;
    the row sums of weight, moment and count; the taps of sigma_a"""
    sh, sw = d["BMTH"] + 4, d["BMTW"] + 4
    cells = (d["BMTH"] // bm.CELL) * (d["BMTW"] // bm.CELL)
    return 4 * ((sh + 2 * r) * (sw + 2 * r) + 2 * (sh + 2 * r) * sw + 2 * sh * sw + 3 * cells * bm.CELL + 2 * bm.MAX_RADIUS + 1)


def test_blur_map_kernels_use_no_scratch_and_fit_a_cu_twice_at_the_largest_radius(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_blurmap.hip")).read()
    assert sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))) == ["k_img_bm"]
    names = ["k_img_bm<%d>" % r for r in RADII]                              # a kernel per radius of sigma_b
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k.startswith("k_img_bm")}
    assert sorted(found) == names, sorted(found)
    d = {m: int(v) for m, v in re.findall(r"#define (BMTW|BMTH|BMLANES) (\d+)", src)}
    assert d == {"BMTW": 64, "BMTH": 32, "BMLANES": 512}
    # the launcher: two workgroups per CU, each two waves per SIMD: four waves per SIMD share its 512 registers
    assert re.search(r"long grid = \(long\)\(cus > 0 \? cus : 256\) \* 2;", src)
    per_cu = 2
    waves_per_simd = per_cu * d["BMLANES"] // 64 // 4
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
        assert v["vgpr_count"] <= 512 // waves_per_simd, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    inner = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_kernels.h")).read()
    for text in (header, inner):
        assert int(re.search(r"#define ICS_IMG_BLURMAP_MAX_RADIUS (\d+)", text).group(1)) == bm.MAX_RADIUS == 8
        assert int(re.search(r"#define ICS_IMG_BLURMAP_CELL (\d+)", text).group(1)) == bm.CELL == 16
    # all of the LDS is dynamic, set by the launcher from this expression
    lds = lds_table(tmp_path)
    assert lds == {k: 0 for k in names}, lds
    assert re.search(r"return \(\(size_t\)\(BMSH \+ 2 \* r\) \* \(BMSW \+ 2 \* r\) \+ \(size_t\)2 \* \(BMSH \+ 2 \* r\) \* BMSW \+ \(size_t\)2 \* BMSH \* BMSW \+ BMROWS \+ 2 \* BMR \+ 1\) "
                     r"\* sizeof\(float\);", src)
    assert "#define BMSH (BMTH + 4)" in src and "#define BMSW (BMTW + 4)" in src and "#define BMROWS (3 * BMCELLS * BMCELL)" in src
    assert lds_bytes(d, 8) == 66948 and lds_bytes(d, 6) == 62660              # the figures of DESIGN.md
    assert per_cu * lds_bytes(d, bm.MAX_RADIUS) <= LDS_PER_CU < (per_cu + 1) * lds_bytes(d, bm.MAX_RADIUS)
