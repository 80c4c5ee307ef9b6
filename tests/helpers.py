"""Shared helpers for the parity tests (numpy only; the oracle lives in oracle/)."""
import json
import os

import numpy as np

import rl_mm_oracle as orc

# oracle/make_golden_levels.py: the pyramid levels the fp16-split matrix cores serve under ICS_CONV_AUTO
LEVEL_FIXTURES = ["nb_2048_k7", "nb_1448_k5", "nb_1024_k3", "nb_1448_k11", "nb_1061x1414_k9_corr", "bl_1024_k7", "nb_1024_k5_stop"]


def load_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "rl_%s.npz" % name))
    meta = json.loads(str(z["meta"]))
    return z, meta


def rel_err(a, b):
    """max |a-b| / max |b| (the '1e-4 relative' of the north star is on this norm)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))


def conv_valid64(u, psf):
    return np.stack([orc._conv_direct(u[..., c], psf[..., c], "valid") for c in range(3)], axis=-1)


def corr_full64(e, psf):
    rot = psf[::-1, ::-1]
    return np.stack([orc._conv_direct(e[..., c], rot[..., c], "full") for c in range(3)], axis=-1)


def gradk64(u, e):
    urot = u[::-1, ::-1]
    return np.stack([orc._conv_direct(urot[..., c], e[..., c], "valid") for c in range(3)], axis=-1)


def update_f32(u, ut, g_raw, image, step, lambd, blind, pad, maxima=False):
    """A5-A10 in numpy float32 with the reference's rounding (lib/deconvolution.pyx:499-552).  Returns (u, dt, DoF), with `maxima` also
    the per-channel max u and max |g| the step sizes were taken from."""
    F = np.float32
    step, lambd = F(step), F(lambd)
    M, N = image.shape[:2]
    inter = (slice(pad, pad + M), slice(pad, pad + N))
    with np.errstate(divide="ignore", invalid="ignore"):
        gi = g_raw[inter]
        DoF = orc.dof_ratio(gi, image) ** 2      # 0/0 -> 1: include/ics_hip.h "DoF ratio"
        if not blind:
            DoF = DoF / lambd
        g = ((lambd * g_raw).astype(np.float64) + (u - ut).astype(np.float64) / 2.0).astype(np.float32)
        dt, maxu, maxg = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        for k in range(3):
            maxu[k], maxg[k] = np.amax(u[..., k]), np.amax(np.abs(g[..., k]))
            dt[k] = F(step * maxu[k]) / F(maxg[k] + F(1e-15))
        un = u.copy()
        for k in range(3):
            un[..., k] -= dt[k] * g[..., k]
        un[inter] = (F(1.0) - DoF) * un[inter] + DoF * image
    return (un, dt, DoF, maxu, maxg) if maxima else (un, dt, DoF)


def psf_step_f32(psf, gradk, step, MK, correlation):
    """A14-A17 in numpy float32 (lib/deconvolution.pyx:574-589).  Returns (local psf, caller's psf)."""
    F = np.float32
    dtpsf = F(F(F(step) / F(MK)) * np.amax(psf)) / F(np.amax(np.abs(gradk)) + F(1e-15))
    p = psf - dtpsf * gradk
    caller = p.copy()
    if correlation:
        m = np.mean(p, axis=2)
        p = np.ascontiguousarray(np.dstack((m, m, m)), dtype=np.float32)
        orc.normalize_kernel(p, MK)
        return p, caller, dtpsf
    orc.normalize_kernel(p, MK)
    return p, p.copy(), dtpsf


_large = {}


def large_case(meta):
    """orc.synth_case_large inputs of a fixture made by oracle/make_golden_{baseline,deep,levels}.py (one problem cached at a time)"""
    key = (meta["M"], meta["N"], meta["MK"], meta["seed"], meta["blind"])
    if key not in _large:
        _large.clear()                      # one full-size problem in host memory at a time
        _large[key] = orc.synth_case_large(meta["M"], meta["N"], meta["MK"], seed=meta["seed"], blind=bool(meta["blind"]))
    return _large[key]


def compare_samples(z, meta, tag, u, psf, gate, sums_tol):
    """u and psf after a run against a sampled fixture (oracle/make_golden_deep.py keep()): crops, every n-th row and column of u
    and the PSF within `gate` relative (of max |u_ref|), float64 moments and quadrant sums of the whole frame within `sums_tol`.
    Returns (worst u error, psf error)."""
    w = meta["where"]
    c, s = w["centre"], w["seam"]
    got = dict(centre=u[c[0]:c[1], c[2]:c[3]], seam=u[s[0]:s[1], s[2]:s[3]], corner=u[-w["corner"]:, -w["corner"]:], origin=u[:w["origin"], :w["origin"]])
    if "u_rows_%s" % tag in z.files:
        got.update(rows=u[::meta["row_step"]], cols=u[:, ::meta["row_step"]])
    den = float(z["moments_%s" % tag][3])                               # max of the reference's u
    errs = {k: float(np.max(np.abs(v.astype(np.float64) - z["u_%s_%s" % (k, tag)]))) / den for k, v in got.items()}
    ep = rel_err(psf, z["psf_%s" % tag])
    uf = u.astype(np.float64)
    mom = np.array([uf.sum(), (uf ** 2).sum(), uf.min(), uf.max()])
    h2, w2 = uf.shape[0] // 2, uf.shape[1] // 2
    quad = np.array([[uf[a:a + h2, b:b + w2, ch].sum() for ch in range(3)] for a in (0, h2) for b in (0, w2)])
    assert max(errs.values()) < gate, (tag, errs)
    assert ep < gate, (tag, ep)
    assert np.all(np.abs(mom - z["moments_%s" % tag]) <= sums_tol * np.abs(z["moments_%s" % tag]))
    assert np.all(np.abs(quad - z["quadrants_%s" % tag]) <= sums_tol * np.abs(z["quadrants_%s" % tag]))
    return max(errs.values()), ep


def lds_table(tmp_path, prefix):
    """static LDS bytes of every gfx950 kernel of the cross-compiled library whose name holds `prefix`, by demangled name (read from the
    AMDGPU metadata as tests/test_mask_isa.py reads it: the size stands in front of the name)"""
    import re
    import shutil
    import subprocess
    from test_isa import LLVM
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    work = tmp_path / "lds"
    work.mkdir()
    shutil.copy(os.path.join(root, "image-cases-studies_amd", "libics_hip.so"), work / "lib.so")
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
            elif m and prefix in m.group(2):
                rows[m.group(2)] = pending
    names = subprocess.check_output(["c++filt"], input="\n".join(rows), text=True).splitlines()
    return {nice.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]: rows[mangled] for mangled, nice in zip(rows, names)}


def log_numbers(line):
    return [float(t) for t in line.replace("|", " ").replace("=", " ").split() if t.replace(".", "").replace("-", "").isdigit()]


def assert_log_matches(log, ref_log, rtol):
    """the reference's own progress lines, line for line; a line that differs may differ only in its printed numbers (DoF extrema and
    statistics printed with six decimals), within `rtol` / 2e-6 absolute"""
    lines, ref = log.splitlines(), ref_log.splitlines()
    assert len(lines) == len(ref), (lines, ref)
    for lg, lr in zip(lines, ref):
        if lg != lr:
            vg, vr = log_numbers(lg), log_numbers(lr)
            assert len(vg) == len(vr) and np.allclose(vg, vr, rtol=rtol, atol=2e-6), (lg, lr)
