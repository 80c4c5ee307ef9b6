"""CPU: the gfx950 code of csrc/ics_img_tvmdeconv.hip declares exactly the kernels DESIGN.md names ("Masked TV deconvolution on a
resident frame"), uses no scratch memory and spills nothing, its line kernels fit four waves a SIMD, and its LDS is what DESIGN.md
states: the line kernels take theirs at launch (two buffers of one line), the shrink pass static tiles of u and p, the setup and the
count pass one word a lane; the tables and the transposes are the Wiener unit's kernels (read from the AMDGPU metadata of the
cross-compiled library like tests/test_tv_deconv_isa.py: metadata only, no instruction is searched for)."""
import os
import re
import shutil
import subprocess

import wiener_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
LINE_KERNELS = ["k_img_tvm_blur_cols", "k_img_tvm_cols", "k_img_tvm_inv_rows", "k_img_tvm_psf_cols", "k_img_tvm_psf_rows", "k_img_tvm_rows"]
OTHER_KERNELS = ["k_img_tvm_count", "k_img_tvm_setup", "k_img_tvm_shrink"]      # (the tables and the transposes are the Wiener unit's kernels)


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
            elif m and "k_img_tvm_" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


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
    for own in ("ics_img_tvdeconv.hip", "ics_img_wiener.hip"):                         # ... and those units declare no kernel of this one
        assert "k_img_tvm_" not in open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", own)).read()
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k.split("<")[0] in declared}
    assert sorted(set(k.split("<")[0] for k in found)) == declared, sorted(found)
    assert sorted(k for k in found if "<" in k) == ["k_img_tvm_shrink<false>", "k_img_tvm_shrink<true>"]
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    # a line's workgroup has up to 1024 lanes, 16 waves, four per SIMD: at most 512 / 4 registers
    for k in LINE_KERNELS:
        assert found[k]["vgpr_count"] <= 128, (k, found[k])
    # LDS: the shrink pass holds u on its 16 x 64 tile and one pixel around it and px, py on the tile and one pixel above and left of
    # it, three channels each; the setup 256 ints and the count 256 64-bit sums; every line kernel takes 2 P float2 at launch and
    # nothing static
    d = {m: int(v) for m, v in re.findall(r"#define (TVM_LANES|TVM_PER|TVM_TW|TVM_TH) (\d+)", src)}
    assert d == {"TVM_LANES": 1024, "TVM_PER": 8, "TVM_TW": 64, "TVM_TH": 16}
    assert d["TVM_LANES"] * d["TVM_PER"] == wr.MAX_SIDE                                # the column kernel holds a whole line in its lanes
    shrink = 4 * 3 * (18 * 66 + 2 * 17 * 65)
    assert shrink == 40776
    lds = lds_table(tmp_path)
    assert sorted(lds) == sorted(found)
    for k, v in lds.items():                                                           # (the code object rounds the two arrays up to 16 bytes)
        want = (shrink + 15) // 16 * 16 if k.startswith("k_img_tvm_shrink") else {"k_img_tvm_setup": 1024, "k_img_tvm_count": 2048}.get(k, 0)
        assert v == want, (k, v)
    assert "`12 · (18 · 66 + 2 · 17 · 65) = 40 776 B`" in section and "`16 P` bytes" in section and "1 024 B" in section and "2 048 B" in section
    assert "ics_img_wiener_lds(Py)" in src and "ics_img_wiener_lds(ICS_IMG_WIENER_MAX)" in src        # the line kernels' launch-time LDS
    assert 16 * wr.MAX_SIDE == 128 * 1024 <= LDS_PER_CU
    assert "getenv" not in src
