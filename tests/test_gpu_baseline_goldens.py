"""Reference trajectories at the frame sizes BASELINE.json's metric is quoted on (oracle/make_golden_baseline.py): the COMPILED
REFERENCE (lib/deconvolution.pyx:460-659 itself, not a float64 stage pass) ran configs[1] -- non-blind 2048^2, 15 x 15, two outer
iterations --, the blind loop at 2048^2 (two outer iterations), one outer iteration of configs[2] -- blind 4096^2, 15 x 15, the
headline workload -- and one of configs[3] -- blind 6144^2, 31 x 31 (two-window 8-wave convolutions, 2 x 2 tap-block gradient); the fixtures keep crops (centre, a corner shared by four 64 x 64 tiles, frame corner, frame origin), every n-th
row and column, float64 moments and quadrant sums of the whole frame, the PSF and the reference's stdout.  Here the product path
runs the same calls on the full grid with the default kernels, with fp32 products (`conv=1`) and on the fp16-split matrix cores
(`conv=2`, which AUTO no longer picks at 4096^2 and above); gate = 1e-5 on u and on the PSF
(the north-star bar is 1e-4), the whole-frame sums to 1e-6."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from helpers import assert_log_matches, compare_samples, large_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("conv", [pytest.param(0, id="default-kernels"), pytest.param(1, id="fp32-products"), pytest.param(2, id="matrix")])
@pytest.mark.parametrize("name", ["nb_2048_k15", "bl_2048_k15", "bl_4096_k15", "bl_6144_k31"])
def test_reference_trajectory_at_baseline_size(golden_dir, name, conv):
    from lib import deconvolution as dc
    z = np.load(os.path.join(golden_dir, "rl_%s.npz" % name))
    meta = json.loads(str(z["meta"]))
    M, N, MK = meta["M"], meta["N"], meta["MK"]
    case = large_case(meta)
    dc._drop_jobs()
    for n in meta["iters"]:
        u, psf = case["u0"].copy(), case["psf0"].copy()
        image = case["image"].copy()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = dc.richardson_lucy_MM(image, u, psf, *meta["window"], meta["tau"], M, N, 3, MK, n, meta["step"], meta["lambd"],
                                        blind=bool(meta["blind"]), conv=conv)
        st = dc.richardson_lucy_MM.last
        assert np.shares_memory(out, u) and st.iterations_done == n and not st.has_nan
        assert np.array_equal(image, case["image"])                       # pyx:545-549 subtract exactly 0
        eu, ep = compare_samples(z, meta, str(n), u, psf, 1e-5, 1e-6)
        print("%s conv=%d, %d outer: u %.2e psf %.2e" % (name, conv, n, eu, ep))
        # the reference's own progress lines (DoF extrema printed with six decimals may differ in the last digit)
        assert_log_matches(buf.getvalue(), meta["logs"][str(n)], 2e-4)
        if "M_r" in z.files:
            k = st.trace_len
            np.testing.assert_allclose(np.array(st.trace_M_r[:k]), z["M_r"][:k], rtol=5e-3)
            np.testing.assert_allclose(np.array(st.trace_Hu[:k]), z["Hu"][:k], rtol=5e-3)
            np.testing.assert_allclose(np.array(st.trace_varu[:k]), z["varu"][:k], rtol=1e-3)
    dc._drop_jobs()
