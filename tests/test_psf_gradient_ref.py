"""CPU: the references, gates and mutants of tests/test_gpu_psf_gradient.py (tests/psf_gradient_ref.py) -- no device code runs here.

  * the float64 form through float64 FFTs agrees with the direct sums to 1e-12 on each convolution of the loop;
  * the inputs replayed for the mutants give the recorded gradient bit for bit;
  * for every case of the GPU module every mutant lies at least 10 gates from the reference.  A condition, not a measurement: a case that
    misses it gets another seed, the factors stay;
  * every case routes where the GPU module says (ics_describe needs no device), both geometry classes hold all fifteen compiled PSF sizes of
    the small-frame kernel, and the cases contain every PSF-gradient family of a blind shipped-loop run;
  * why the module exists: on the cases of tests/test_gpu_small.py a transposed gradient and one that lacks a tile's share stay inside the
    whole-run gates on u, the PSF and the traces."""
import numpy as np
import pytest

import psf_gradient_ref as pg
import rl_mm_oracle as orc
import route_cases as rc
import test_gpu_psf_gradient as gp


def test_float64_ffts_agree_with_the_direct_sums():
    c = pg.case(40, 52, 7, seed=3)
    rng = np.random.default_rng(5)
    e = rng.standard_normal((c.M, c.N)) * 1e-2
    u = c.u0[..., 1].astype(np.float64)
    k = c.psf0[..., 1].astype(np.float64)
    for a, b, mode in ((u, k, "valid"), (e, k[::-1, ::-1], "full"), (u[::-1, ::-1], e, "valid")):       # A1 / A11, A3, A13
        d, f = orc._conv_direct(a, b, mode), orc._conv_fft64(a, b, mode)
        assert d.shape == f.shape and np.abs(f - d).max() <= 1e-12 * np.abs(d).max(), (mode, np.abs(f - d).max() / np.abs(d).max())
    # a whole outer iteration: float32 arrays either way, so the two forms part by roundings of values within 1e-12 of a tie, no more
    g_d, dt_d = pg.last_gradient(c, form="direct")
    g_f, dt_f = pg.last_gradient(c, form="fft64")
    print("last gradient, float64 FFTs against direct sums: %.2e" % pg.rel(g_f, g_d))
    assert pg.rel(g_f, g_d) <= 4 * np.finfo(np.float32).eps and abs(float(dt_f) / float(dt_d) - 1) <= 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("correlation,iterations", [(0, 1), (1, 1), (0, 2)])
def test_replayed_inputs_give_the_recorded_gradient(correlation, iterations):
    c = pg.case(33, 41, 5, seed=1)
    u, e = pg.inputs(c, None, correlation, iterations)          # (asserts the bit equality itself)
    assert u.shape == c.u0.shape and e.shape == c.image.shape and np.abs(e).max() > 0
    assert len(pg._run(c, pg.small_window(c), "direct", correlation, iterations)[0].gradk) == 5 * iterations


def test_case_arrays_are_read_only_and_the_psf_has_no_symmetry():
    c = pg.case(33, 41, 5, seed=1)
    for a in (c.image, c.u0, c.psf0):
        assert not a.flags.writeable and a.dtype == np.float32
    p = c.psf0
    assert np.allclose(p.sum(axis=(0, 1)), 1, atol=1e-6)
    for q in (p.transpose(1, 0, 2), p[::-1, ::-1], p[..., [1, 0, 2]]):
        assert np.abs(q - p).max() > 0.1 * p.max()


@pytest.mark.parametrize("g", gp.all_cases(), ids=lambda g: g.id)
def test_every_mutant_is_ten_gates_away(g):
    c = gp.data(g)
    gate = gp.gate_of(g)          # 8 D; 4 x the float32 restatement for the cases of gp.F32_GATED
    sep = pg.separations(c, None, g.correlation, g.iterations)
    w = min(sep, key=sep.get)
    print("%-62s D %.2e gate %.2e weakest: %s %.2e = %.1f gates" % (g.id, pg.D(c, None, g.correlation, g.iterations), gate, w, sep[w], sep[w] / gate))
    assert gate > 0 and len(sep) >= 10
    assert ("tiles past 64 missing" in sep) == (np.prod(pg.tiles(c)) > pg.LANES)
    for name, s in sep.items():
        assert s >= pg.FLOOR * gate, (g.id, name, s, gate)


def test_one_ulp_of_the_psf_scale_explains_the_restated_gate():
    """the finding behind gp.F32_GATED: float32 direct sums are either 3e-6 from the float64 form or one ulp of the PSF's scale away,
    depending on nothing but the order of the taps; the complex64 form (D) happened to stay on the float64 form's side"""
    assert set(gp.F32_GATED) <= {g.id for g in gp.all_cases()}
    for g in gp.all_cases():
        if g.id not in gp.F32_GATED:
            continue
        c = gp.data(g)
        ref = pg.last_gradient(c, None, "float64", g.correlation, g.iterations)[0]
        r = {form: pg.rel(pg.last_gradient(c, None, form, g.correlation, g.iterations)[0], ref) for form in pg.FORMS}
        ulp, d = pg.psf_scale_term(c, None, g.correlation, g.iterations), pg.D(c, None, g.correlation, g.iterations)
        print("%s: float32 direct sums %s, one ulp of the PSF scale %.2e, D %.2e" % (g.id, {k: "%.2e" % v for k, v in r.items()}, ulp, d))
        assert min(r.values()) < 0.1 * ulp and 0.5 * ulp < max(r.values()) < 2 * ulp and d < 0.25 * ulp


def test_cases_route_where_they_claim_and_cover_every_family():
    from lib import _native as nv
    for g in gp.all_cases():
        old = {k: nv.debug_set(k, v) for k, v in dict(dict(rc.SWITCH_DEFAULTS, fft_psf1=1), **dict(g.switches)).items()}
        try:
            p = nv.RLJob.params(*g.win, 1e9, g.iterations, pg.STEP, pg.LAMBD, True, g.correlation, 3, stop_test=1, fuse=g.fuse, conv=g.conv, flags=g.flags)
            r = nv.describe(g.M, g.N, g.MK, p)
        finally:
            for k, v in old.items():
                nv.debug_set(k, v)
        assert (r.conv_family, r.gradk_family) == (g.conv_family, g.gradk_family), (g.id, r.conv_family, r.gradk_family)
    for name, f in (("exact", gp.exact), ("over-under", gp.over_under)):
        sizes = [g.MK for g in gp.SMALL if g.group == "small " + name]
        assert sizes == list(range(3, 32, 2))
        for g in gp.SMALL:
            if g.group == "small " + name:
                assert (g.M, g.N) == f(g.MK) and min(g.M, g.N) > g.MK and g.conv_family == 6
    uM, uN = gp.exact(31)[0] + 30, gp.exact(31)[1] + 30
    assert (uM % 32, uN % 32) == (0, 0) and ((gp.over_under(31)[0] + 30) % 32, (gp.over_under(31)[1] + 30) % 32) == (1, 31)
    here = {g.gradk_family for g in gp.all_cases()}
    assert here >= gp.families_everywhere() and here == set(gp.GK)
    auto = {(g.conv_family, g.gradk_family) for g in gp.all_cases()}
    assert {(6, 8), (5, 7), (1, 1)} <= auto          # what ICS_CONV_AUTO picks: the small kernel, the fused tile unit, the fused matrix-core unit


# ---- why the module exists ----------------------------------------------------------------------------------------------------------------
def _whole_run(M, N, MK, iters, mutate):
    """the case of tests/test_gpu_small.py::test_whole_run_against_the_oracle with A13 replaced by mutate(u_rot, error) -> gradient"""
    case = orc.synth_case(M, N, MK, seed=11, blind=True)
    win = orc.default_window(M, N, MK) if min(M, N) > 3 * MK + 8 else (1, M - 1, 1, N - 1)

    def cv(a, b, mode):
        if mode == "valid" and b.shape == (M, N):            # A13 is the only convolution whose second operand is the residual
            return mutate(a, b)
        return orc._conv_scipy(a, b, mode)

    u, psf = case["u0"].copy(), case["psf0"].copy()
    tr = orc.Trace()
    with np.errstate(all="ignore"):
        orc.richardson_lucy_MM(case["image"].copy(), u, psf, *win, 1e9, M, N, 3, MK, iters, 1e-3, 10000.0, blind=True, conv=cv, trace=tr,
                               quiet=True, dof_zero_rule=float("nan"))
    return u, tr.psf_final, tr


@pytest.mark.parametrize("M,N,MK,iters", [(97, 64, 3, 3), (200, 131, 5, 3)])
def test_the_whole_run_gates_do_not_see_a_wrong_gradient(M, N, MK, iters):
    pad = MK // 2

    def right(a, b):
        return orc._conv_scipy(a, b, "valid")

    def transposed(a, b):
        return right(a, b).T

    def tile_missing(a, b):
        b = b.copy()
        b[32 - pad:64 - pad, 32 - pad:64 - pad] = 0          # the residual pixels of tile (1, 1) of the u-frame
        return right(a, b)

    u0, psf0, tr0 = _whole_run(M, N, MK, iters, right)
    for name, f in (("transposed", transposed), ("a tile's share missing", tile_missing)):
        u, psf, tr = _whole_run(M, N, MK, iters, f)
        assert pg.rel(tr.gradk[-1], tr0.gradk[-1]) > 1e-2, name          # the gradient is wrong ...
        eu, ep = pg.rel(u, u0), pg.rel(psf, psf0)
        print("%d x %d / %d, %s: u %.2e psf %.2e of max |ref| (gate 1e-4)" % (M, N, MK, name, eu, ep))
        assert 0 < ep <= 1e-4 and eu <= 1e-4, (name, eu, ep)               # ... and every whole-run gate of tests/test_gpu_small.py holds
        for t in ("M_r", "Hu", "varu", "dof_min", "dof_max"):
            assert np.allclose(np.array(getattr(tr, t), np.float64), np.array(getattr(tr0, t), np.float64), rtol=2e-3, atol=1e-7, equal_nan=True), (name, t)
