"""CPU: the gfx950 code of csrc/ics_img_llf.hip uses no scratch memory and spills no register (read from the AMDGPU metadata of the
cross-compiled library like tests/test_isa.py), the LDS of its reduce kernels is what the unit's comment states, and its registers
leave the occupancy DESIGN.md ("Local Laplacian on a resident frame") claims: 64 VGPRs or fewer, so the 8 waves per SIMD the hardware
allows, and the LDS alone decides how many workgroups of 256 lanes share a CU -- three of the batched level-0 kernel."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lds_bytes(planes):
    """csrc/ics_img_llf.hip: `planes` input planes of 67 rows and one scratch plane of 32 rows, row stride 68 floats"""
    return 4 * (planes * 67 + 32) * 68


def lds_table(work, llvm):
    """static LDS bytes by mangled kernel name from the code objects kernel_table unpacked into `work`.  The metadata lists a
    kernel's keys in alphabetical order, .group_segment_fixed_size before .name, so kernel_table (which files every key under the
    name it saw last) files that one key under the kernel before; here a value waits for the .name that follows it."""
    out = {}
    for f in sorted(os.listdir(work)):
        if not f.endswith("gfx950"):
            continue
        pending = None
        for line in subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", f], cwd=work, text=True).splitlines():
            m = re.match(r"    \.(group_segment_fixed_size|name):\s+(\S+)", line)      # the kernel's own keys: four spaces
            if m and m.group(1) == "name":
                out[m.group(2)], pending = pending, None
            elif m:
                pending = int(m.group(2))
    return out


def test_llf_kernels_use_no_scratch_and_their_lds_is_the_stated_formula(tmp_path):
    from test_isa import LLVM, kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_llf.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_llf_collapse", "k_img_llf_reduce", "k_img_llf_reduce0", "k_img_llf_reduce0_batched"]
    tab = kernel_table(tmp_path)
    found = {}
    for name in declared:
        rows = {k: v for k, v in tab.items() if k == name or k.startswith(name + "<")}
        assert rows, "%s is not in the code object" % name
        found.update(rows)
        for k, v in rows.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    assert sorted(found) == ["k_img_llf_collapse<false, false>", "k_img_llf_collapse<false, true>", "k_img_llf_collapse<true, true>", "k_img_llf_reduce",
                             "k_img_llf_reduce0<false>", "k_img_llf_reduce0<true>", "k_img_llf_reduce0_batched<false>", "k_img_llf_reduce0_batched<true>"]
    mangled = lds_table(str(tmp_path / "co"), LLVM)
    names = subprocess.check_output(["c++filt"], input="\n".join(mangled), text=True).splitlines()
    static_lds = {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: mangled[m] for m, nice in zip(mangled, names)}
    print({k: (v["vgpr_count"], v["sgpr_count"], static_lds[k]) for k, v in found.items()})
    tile = {m: int(v) for m, v in re.findall(r"#define (LLT|LLIN|LLS|LLLANES) (\d+)", src)}
    assert tile == {"LLT": 32, "LLIN": 67, "LLS": 68, "LLLANES": 256} and tile["LLIN"] == 2 * tile["LLT"] + 3
    lds = 160 * 1024
    for k, v in found.items():
        assert v["vgpr_count"] <= 64, (k, v)                              # 8 waves per SIMD: registers never limit the occupancy
        want = 0 if "collapse" in k else lds_bytes(2) if "batched" in k else lds_bytes(1)
        assert static_lds[k] == want, (k, static_lds[k], want)
    # the unit's comment and DESIGN.md: 26 928 B and 45 152 B, six and three workgroups per CU
    assert (lds_bytes(1), lds_bytes(2)) == (26928, 45152) and (lds // lds_bytes(1), lds // lds_bytes(2)) == (6, 3)
