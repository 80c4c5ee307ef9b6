"""CPU: the gfx950 code of csrc/ics_img_despeckle.hip uses no scratch memory and spills nothing (read from the AMDGPU metadata of the
cross-compiled library like tests/test_isa.py), its static LDS is the tile arithmetic DESIGN.md states ("Despeckle on a resident
frame"), and its registers leave room for the workgroups per CU its launch bounds name."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024


def lds_table(tmp_path):
    """static LDS bytes per kernel of this unit.  (In the metadata .group_segment_fixed_size stands in front of the kernel's .name;
    test_isa.kernel_table files what it reads under the name it met last.)"""
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
            m = re.match(r"    \.(group_segment_fixed_size|name):\s+(\S+)", line)      # kernel level: four spaces (arguments sit deeper)
            if m and m.group(1) == "group_segment_fixed_size":
                pending = int(m.group(2))
            elif m and "k_img_ds_" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def test_despeckle_kernels_use_no_scratch_and_their_tiles_are_what_the_design_states(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_despeckle.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_ds_direct", "k_img_ds_tile"]
    tab = kernel_table(tmp_path)
    found = {}
    for name in declared:
        rows = {k: v for k, v in tab.items() if k == name or k.startswith(name + "<")}
        assert rows, "%s is not in the code object" % name
        found.update(rows)
        for k, v in rows.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    # templated on radius and coupling (<false> is "channel")
    assert sorted(found) == sorted("%s<%d, %s>" % (k, r, v) for k in declared for r in (1, 2) for v in ("false", "true"))
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    d = {m: int(v) for m, v in re.findall(r"#define (DST|DSP|DSLANES|DSWAVE|DSWGS) (\d+)", src)}
    assert d == {"DST": 32, "DSP": 4, "DSLANES": 256, "DSWAVE": 64, "DSWGS": 4} and d["DST"] * (d["DST"] // d["DSP"]) == d["DSLANES"]
    assert len(re.findall(r"__launch_bounds__\(DS(?:WAVE|LANES), DSWGS\)", src)) == 2
    lds = lds_table(tmp_path)
    assert sorted(lds) == sorted(found), lds
    tile = {r: 4 * (3 * (d["DST"] + 2 * r) ** 2 + 3) for r in (1, 2)}         # three planes of keys, tile + halo, and three counters
    assert tile == {1: 13884, 2: 15564}
    for k, v in found.items():
        r = int(k.split("<")[1][0])
        assert lds[k] == (tile[r] if k.startswith("k_img_ds_tile") else 0), (k, lds[k])                  # route 1: no LDS at all
        # the launch bounds: DSWGS waves per SIMD, that is DSWGS workgroups of 256 lanes (one wave per SIMD each) per CU, 512 registers a lane and SIMD
        assert v["vgpr_count"] <= 512 // d["DSWGS"] == 128, (k, v)                                       # no kernel above 128 registers
        assert d["DSWGS"] * lds[k] <= LDS_PER_CU
    assert LDS_PER_CU // tile[2] == 10                                                                  # LDS never limits: registers do
