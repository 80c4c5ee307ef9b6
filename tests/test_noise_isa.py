"""CPU: the gfx950 code of csrc/ics_img_noise.hip uses no scratch memory (read from the AMDGPU metadata of the cross-compiled library
like tests/test_isa.py), its LDS is the tile and histogram arithmetic DESIGN.md states ("Noise estimate on a resident frame"), and its
registers leave room for the workgroups per CU its launcher sizes the persistent grids by."""
import os
import re
import shutil
import subprocess

import noise_ref  # noqa: F401  (the specification these kernels implement: without it there is nothing to check)

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
            elif m and "k_img_ns_" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def test_noise_kernels_use_no_scratch_and_fit_as_often_as_their_grids_assume(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_noise.hip")).read()
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == ["k_img_ns_hist", "k_img_ns_keys", "k_img_ns_recompute", "k_img_ns_select"]
    tab = kernel_table(tmp_path)
    found = {}
    for name in declared:
        rows = {k: v for k, v in tab.items() if k == name or k.startswith(name + "<")}
        assert rows, "%s is not in the code object" % name
        found.update(rows)
        for k, v in rows.items():
            assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    assert sorted(found) == ["k_img_ns_hist<false>", "k_img_ns_hist<true>", "k_img_ns_keys<false>", "k_img_ns_keys<true>",
                             "k_img_ns_recompute<false>", "k_img_ns_recompute<true>", "k_img_ns_select"]
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    lds = lds_table(tmp_path)
    assert sorted(lds) == sorted(found), lds
    d = {m: int(v) for m, v in re.findall(r"#define (NSB0|NSB1|NSLANES|NSTW|NSTH|NSHK) (\d+)", src)}
    assert d == {"NSB0": 11, "NSB1": 10, "NSLANES": 256, "NSTW": 64, "NSTH": 16, "NSHK": 4} and d["NSB0"] + 2 * d["NSB1"] == 31
    # per population bins x 2 counters x 4 B: 2048 bins where the first pass runs, 1024 in the kernel of the later passes; <false> is "channel"
    hist = {False: 3 * 2 ** d["NSB0"] * 2 * 4, True: 2 ** d["NSB0"] * 2 * 4}
    hist_later = {False: 3 * 2 ** d["NSB1"] * 2 * 4, True: 2 ** d["NSB1"] * 2 * 4}
    tile = 4 * 4 * (d["NSTW"] + 4) * (d["NSTH"] + 4)                              # three planes of c_0 and one of the row pass, 68 x 20 floats
    assert hist == {False: 49152, True: 16384} and hist_later == {False: 24576, True: 8192} and tile == 21760
    for vec, name in ((False, "<false>"), (True, "<true>")):
        # static LDS: the histograms; the keys kernel's is dynamic (tile + histograms, set by the launcher)
        assert lds["k_img_ns_recompute" + name] == hist[vec], lds
        assert lds["k_img_ns_hist" + name] == hist_later[vec], lds
        assert lds["k_img_ns_keys" + name] == 0, lds
    assert lds["k_img_ns_select"] == 4 * d["NSLANES"] // 64, lds
    assert re.search(r"return \(size_t\)4 \* NSN \* sizeof\(float\) \+ \(size_t\)\(coupling \? 1 : 3\) \* NSBINS \* 2 \* sizeof\(unsigned\);", src)
    # the launcher's persistent grids, workgroups of 256 lanes per CU ("channel", "vector")
    m = re.search(r"const int rec_per_cu = coupling \? (\d) : (\d), keys_per_cu = coupling \? (\d) : (\d), hist_per_cu = (\d);", src)
    per_cu = {"k_img_ns_recompute": {True: int(m.group(1)), False: int(m.group(2))}, "k_img_ns_keys": {True: int(m.group(3)), False: int(m.group(4))},
              "k_img_ns_hist": {True: int(m.group(5)), False: int(m.group(5))}}
    assert per_cu == {"k_img_ns_recompute": {True: 4, False: 3}, "k_img_ns_keys": {True: 4, False: 2}, "k_img_ns_hist": {True: 4, False: 4}}
    for vec, name in ((False, "<false>"), (True, "<true>")):
        need = {"k_img_ns_recompute": hist[vec], "k_img_ns_keys": tile + hist[vec], "k_img_ns_hist": hist_later[vec]}
        assert need["k_img_ns_keys"] == {False: 70912, True: 38144}[vec]
        for k, bytes_ in need.items():
            assert per_cu[k][vec] * bytes_ <= LDS_PER_CU, (k, vec)
            # a workgroup is one wave per SIMD: w workgroups per CU are w waves per SIMD, 512 registers per lane and SIMD allow each 512 / w
            assert found[k + name]["vgpr_count"] <= 512 // per_cu[k][vec], (k + name, found[k + name])
            assert found[k + name]["vgpr_count"] <= 128, (k + name, found[k + name])     # no kernel above 128 registers
    assert 3 * (tile + hist[False]) > LDS_PER_CU                                         # "channel": the keys kernel fits twice, not three times
