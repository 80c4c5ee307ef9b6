"""The whole loop at the pyramid levels the fp16-split matrix cores serve (oracle/make_golden_levels.py).

Under ICS_CONV_AUTO the small frames run on the cooperative kernel and the large ones on the transform tiles; everything in
between -- the levels deblur_module walks on an ordinary photo, roughly 0.1 to 12 Mpx with small PSFs -- runs on conv family 1
with conv_fp16_split = 1 (k_conv_mfma, k_synth_gradk / k_gradk_mfma: each operand split into two fp16 terms).  The COMPILED
REFERENCE ran, on orc.synth_case_large inputs,
  * nb_2048_k7, nb_1448_k5, nb_1024_k3   levels 2-4 of a 4096^2 photo with blur 15, non-blind, 2 outer iterations,
  * nb_1448_k11                          level 1 of a 2048^2 photo with blur 15,
  * nb_1061x1414_k9_corr                 non-square, no multiple of any tile edge, correlation=True (the motion-blur branch),
  * bl_1024_k7                           blind: A11 + A13 on the matrix cores at a small PSF,
  * nb_1024_k5_stop                      non-blind with a real tau: the reference's own stop test ends the call, every decision with
                                         a margin >= 1e-3;
tests/test_golden_routes.py pins that AUTO sends every one of them to the matrix cores.  Here each runs under AUTO, with fp32
products (conv=1), on the transform tiles (conv=3), and under AUTO with the 32-row and the 64-row k_conv_mfma tiles forced
(ICS_TEST_CONV_RS 2 / 4; both are built for MK <= 13).  Gate: 1e-5 relative on crops, rows, columns and the PSF, or twice the
fixture's recorded noise floor (float64-direct oracle vs reference) where that is larger, never above the north-star 1e-4; the
whole-frame moments and quadrant sums to 1e-6; the reference's printed lines, stop decision and per-outer scalars."""
import contextlib
import io

import numpy as np
import pytest

from helpers import LEVEL_FIXTURES, assert_log_matches, compare_samples, large_case, load_golden

pytestmark = pytest.mark.gpu

# (conv, forced k_conv_mfma tile height: ICS_TEST_CONV_RS, 0 = the launcher's pick)
RUNS = [pytest.param((0, 0), id="auto"), pytest.param((1, 0), id="fp32"), pytest.param((3, 0), id="fft"),
        pytest.param((0, 2), id="auto-rs32"), pytest.param((0, 4), id="auto-rs64")]


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("name", LEVEL_FIXTURES)
def test_reference_trajectory_at_a_matrix_core_level(golden_dir, debug_switch, name, run):
    from lib import deconvolution as dc
    conv, rs = run
    z, meta = load_golden(golden_dir, name)
    M, N, MK = meta["M"], meta["N"], meta["MK"]
    if rs and MK > 13:
        pytest.skip("only one k_conv_mfma tile height is built for %d x %d" % (MK, MK))
    floor = meta["noise_floor"]
    gate = max(1e-5, 2 * max(floor[0], floor[1]))
    assert gate <= 1e-4, floor
    case = large_case(meta)
    dc._drop_jobs()                      # the tile height is picked when a job is made
    if rs:
        debug_switch("conv_rs", rs)
    tag = meta["tags"][0]
    u, psf = case["u0"].copy(), case["psf0"].copy()
    image = case["image"].copy()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = dc.richardson_lucy_MM(image, u, psf, *meta["window"], meta["tau"], M, N, 3, MK, meta["iters"], meta["step"], meta["lambd"],
                                    blind=bool(meta["blind"]), correlation=bool(meta["corr"]), conv=conv)
    st = dc.richardson_lucy_MM.last
    dc._drop_jobs()
    assert np.shares_memory(out, u) and not st.has_nan
    assert np.array_equal(image, case["image"])                           # pyx:545-549 subtract exactly 0
    assert (st.iterations_done, bool(st.stopped)) == (meta["iterations_done"], meta["stopped"])
    eu, ep = compare_samples(z, meta, tag, u, psf, gate, 1e-6)
    print("%s conv=%d conv_rs=%d, %d outer (stopped=%d): u %.2e psf %.2e (gate %.1e, noise floor %.1e / %.1e)"
          % (name, conv, rs, st.iterations_done, st.stopped, eu, ep, gate, floor[0], floor[1]))
    assert_log_matches(buf.getvalue(), meta["logs"][tag], 2e-4)
    k = st.trace_len
    assert k == meta["iterations_done"] == len(z["M_r"])
    np.testing.assert_allclose(np.array(st.trace_M_r[:k]), z["M_r"], rtol=5e-3)
    np.testing.assert_allclose(np.array(st.trace_Hu[:k]), z["Hu"], rtol=5e-3)
    np.testing.assert_allclose(np.array(st.trace_varu[:k]), z["varu"], rtol=1e-3)
