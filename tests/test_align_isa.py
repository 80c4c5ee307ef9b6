"""CPU: the gfx950 code of csrc/ics_img_align.hip declares exactly the kernels DESIGN.md names ("Registration and warp on a resident
frame"), uses no scratch memory and spills nothing, its sums kernel stays within the register budget DESIGN.md states for every model,
and its LDS is what DESIGN.md states: one row of the slot per lane in the sums kernel (pitch odd), 1024 doubles in the reduction,
none elsewhere (read from the AMDGPU metadata of the cross-compiled library like tests/test_psf_estimate_isa.py: metadata only, no
instruction is searched for)."""
import os
import re
import shutil
import subprocess

import align_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_img_al_half", "k_img_al_luma", "k_img_al_reduce", "k_img_al_sums", "k_img_al_warp"]
VGPR_BUDGET = 128                                                     # four waves a SIMD


def slot(model, photometric):
    n = ar.MODELS[model] + (2 if photometric else 0)
    return n * (n + 1) // 2 + n + 2


def lds_table(tmp_path):
    """static LDS bytes per kernel of this unit (as tests/test_psf_estimate_isa.py reads them: the size stands in front of the name)"""
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
            elif m and "k_img_al_" in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def test_align_kernels_use_no_scratch_and_the_stated_lds_and_registers(tmp_path):
    from test_isa import kernel_table
    assert os.path.isfile(os.path.join(ROOT, "image-cases-studies_amd", "libics_hip.so")), "libics_hip.so is not built"
    src = open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", "ics_img_align.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("**Registration and warp on a resident frame (`csrc/ics_img_align.hip`).**"):]
    section = section[:section.index("\n**", 10)] if "\n**" in section[10:] else section
    declared = sorted(set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src)))
    assert declared == KERNELS
    assert sorted(set(re.findall(r"`(k_img_al_\w+)", section))) == declared                 # DESIGN.md names these and no other
    for other in os.listdir(os.path.join(ROOT, "image-cases-studies_amd", "csrc")):        # ... and no other unit declares one of them
        if other.endswith(".hip") and other != "ics_img_align.hip":
            assert "k_img_al_" not in open(os.path.join(ROOT, "image-cases-studies_amd", "csrc", other)).read(), other
    forms = ["k_img_al_sums<%d, %s>" % (m, p) for m in (0, 1, 2) for p in ("false", "true")]
    names = sorted([k for k in KERNELS if k != "k_img_al_sums"] + forms)
    tab = kernel_table(tmp_path)
    found = {k: v for k, v in tab.items() if k.startswith("k_img_al_")}
    assert sorted(found) == names, sorted(found)
    for k, v in found.items():
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
    print({k: (v["vgpr_count"], v["sgpr_count"]) for k, v in found.items()})
    for k in forms:
        assert found[k]["vgpr_count"] <= VGPR_BUDGET, (k, found[k])
    assert "at most %d vector registers" % VGPR_BUDGET in section
    # LDS: the sums kernel keeps a row of the slot per lane, the pitch made odd; the reduction 1024 doubles
    d = {m: int(v) for m, v in re.findall(r"#define (ALT|ALLANES|ALRED) (\d+)", src)}
    assert d == {"ALT": ar.TILE, "ALLANES": ar.LANES, "ALRED": 1024}
    want = {k: 0 for k in names}
    want["k_img_al_reduce"] = 8 * d["ALRED"]
    for m, model in enumerate(ar.MODELS):
        for p in (False, True):
            want["k_img_al_sums<%d, %s>" % (m, str(p).lower())] = 4 * d["ALLANES"] * (slot(model, p) | 1)
    lds = lds_table(tmp_path)
    assert lds == want, lds
    assert want["k_img_al_sums<2, true>"] == 17152 and want["k_img_al_sums<0, false>"] == 1792
    assert "17 152 B" in section and "1 792 B" in section and "8 192 B" in section
    assert slot("homography", True) == 67 and "67" in section
    assert "getenv" not in src
