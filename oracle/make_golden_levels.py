#!/usr/bin/env python3
"""Reference trajectories at the pyramid levels the fp16-split matrix-core family serves (build container only).

TEST INFRASTRUCTURE ONLY (data, no reference source).  Under ICS_CONV_AUTO the middle range of frame sizes -- roughly 0.1 to
12 Mpx with small PSFs -- runs on conv family 1 with conv_fp16_split = 1 (k_conv_mfma, k_synth_gradk / k_gradk_mfma): the
levels `deblur_module` walks on an ordinary photo, and ordinary richardson_lucy_MM calls.  The COMPILED REFERENCE
(oracle/build_reference.py) runs, on orc.synth_case_large(seed) inputs,

  * nb_2048_k7, nb_1448_k5, nb_1024_k3   non-blind, levels 2-4 of a 4096^2 photo with blur 15, 2 outer iterations;
  * nb_1448_k11                          non-blind, level 1 of a 2048^2 photo with blur 15, 2 outer iterations;
  * nb_1061x1414_k9_corr                 non-blind, correlation=True, a non-square frame that is no multiple of any tile edge;
  * bl_1024_k7                           blind, 2 outer iterations (A11 + A13 on the matrix cores at a small PSF);
  * nb_1024_k5_stop                      non-blind with a real tau: the reference's own stop test ends the call.  tau is picked
                                         from a tau = 1e9 oracle run so that every decision of the call (pyx:643-654) has a
                                         margin |(M_r - M_r_prev) / (M_r + M_r_prev) - tau| >= 1e-3: the case is not fragile.

A fixture keeps what make_golden_deep.py keeps (crops, every n-th row and column, float64 moments and quadrant sums of the whole
frame, the PSF, the reference's stdout) under the tag str(iters), plus the per-outer M_r / Hu / varu of the numpy oracle, which
is asserted equal to the reference bit for bit (arrays and printed lines), the reference's iterations done and stop flag, and
the noise floor: the oracle with float64 direct sums instead of scipy's complex64 FFT, against the reference.

Usage: python oracle/make_golden_levels.py [name ...]"""
import json
import os
import sys
import time

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import build_reference  # noqa: E402
import make_golden as mg  # noqa: E402
import make_golden_deep as md  # noqa: E402
import rl_mm_oracle as orc  # noqa: E402

CASES = [
    dict(name="nb_2048_k7", M=2048, N=2048, MK=7, blind=0, corr=0, iters=2, seed=2007),
    dict(name="nb_1448_k5", M=1448, N=1448, MK=5, blind=0, corr=0, iters=2, seed=1405),
    dict(name="nb_1024_k3", M=1024, N=1024, MK=3, blind=0, corr=0, iters=2, seed=1003),
    dict(name="nb_1448_k11", M=1448, N=1448, MK=11, blind=0, corr=0, iters=2, seed=1411),
    dict(name="nb_1061x1414_k9_corr", M=1061, N=1414, MK=9, blind=0, corr=1, iters=2, seed=1009),
    dict(name="bl_1024_k7", M=1024, N=1024, MK=7, blind=1, corr=0, iters=2, seed=1107),
    dict(name="nb_1024_k5_stop", M=1024, N=1024, MK=5, blind=0, corr=0, iters=8, seed=1205, pick_tau=True),
]

MARGIN = 1e-3


def ratios(M_r):
    """(M_r[i] - M_r[i-1]) / (M_r[i] + M_r[i-1]) in float32 for the decisions i >= 2 (pyx:643-654)"""
    m = np.asarray(M_r, np.float32)
    return {i: float(np.float32(m[i] - m[i - 1]) / np.float32(m[i] + m[i - 1])) for i in range(2, len(m))}


def pick_tau(r):
    """the smallest decision i* >= 3 that can be made the first to fire with every margin >= 2 MARGIN; tau halfway"""
    for i in sorted(r):
        if i < 3:
            continue
        lo, hi = max(r[j] for j in r if j < i), r[i]
        if hi - lo >= 4 * MARGIN:
            return float(np.float32(round((lo + hi) / 2, 6))), i
    raise AssertionError("no decision with a margin >= %g: %s" % (MARGIN, r))


def main():
    ref = build_reference.load()
    want = sys.argv[1:]
    for c in CASES:
        if want and c["name"] not in want:
            continue
        c = dict(c, step=1e-3, lambd=10000.0, tau=1e9)
        M, N, MK = c["M"], c["N"], c["MK"]
        c["row_step"] = 3 * (M // 16) // 2 + 1
        c["window"] = orc.default_window(M, N, MK)
        t0 = time.time()
        case = orc.synth_case_large(M, N, MK, seed=c["seed"], blind=bool(c["blind"]))
        print(c["name"], "inputs %.1f s" % (time.time() - t0), flush=True)
        if c.pop("pick_tau", False):
            t0 = time.time()
            _, _, _, tr = mg.run_orc(case, c, c["iters"])
            r = ratios(tr.M_r)
            c["tau"], fire = pick_tau(r)
            print("  tau = %r (fires at outer iteration %d; ratios %s): %.1f s" % (c["tau"], fire, r, time.time() - t0), flush=True)
        t0 = time.time()
        img_r, u_r, psf_r, log_r = mg.run_ref(ref, case, c, c["iters"])
        print("  reference (%d outer): %.1f s" % (c["iters"], time.time() - t0), flush=True)
        assert np.array_equal(img_r, case["image"])
        t0 = time.time()
        _, u_o, psf_o, tr = mg.run_orc(case, c, c["iters"])
        print("  oracle: %.1f s" % (time.time() - t0), flush=True)
        assert np.array_equal(u_r, u_o) and np.array_equal(psf_r, psf_o) and log_r == tr.log.getvalue(), c["name"]
        if c["tau"] < 1e9:
            assert tr.stopped and tr.iterations < c["iters"], (tr.stopped, tr.iterations)
        if c["blind"] == 0:   # every decision the reference took, with its margin (the blind test M_r > M_r_prev is not used here)
            margins = {i: abs(v - c["tau"]) for i, v in ratios(tr.M_r).items()}
            assert c["tau"] >= 1e9 or min(margins.values()) >= MARGIN, margins
        out = {}
        tag = str(c["iters"])
        where = md.keep(out, tag, u_r, psf_r, c)
        out["M_r"] = np.array(tr.M_r, np.float32)
        out["Hu"] = np.array(tr.Hu, np.float32)
        out["varu"] = np.array(tr.varu, np.float32)
        t0 = time.time()
        _, u_d, psf_d, tr_d = mg.run_orc(case, c, c["iters"], conv="direct")
        noise = [mg.rel(u_d, u_r), mg.rel(psf_d, psf_r), tr_d.iterations]
        print("  float64-direct oracle: %.1f s, noise floor u %.2e psf %.2e" % (time.time() - t0, noise[0], noise[1]), flush=True)
        meta = dict(c, logs={tag: log_r}, where=where, generator="synth_case_large", tags=[tag],
                    iterations_done=tr.iterations, stopped=tr.stopped, noise_floor=noise,
                    versions=dict(numpy=np.__version__, scipy=scipy.__version__, python=sys.version.split()[0],
                                  reference="aurelienpierre/Image-Cases-Studies lib/deconvolution.pyx (cython language_level=2, -O3 -fopenmp)"))
        out["meta"] = np.array(json.dumps(meta))
        path = os.path.join(mg.OUT, "rl_%s.npz" % c["name"])
        np.savez_compressed(path, **out)
        print(path, "%.1f KB, %d outer iterations, stopped=%s" % (os.path.getsize(path) / 1024, tr.iterations, tr.stopped), flush=True)


if __name__ == "__main__":
    main()
