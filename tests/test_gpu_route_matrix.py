"""Every kernel route resolve_route can pick, run as whole calls against the oracle (tests/route_cases.py holds the cases; the CPU test
tests/test_route_coverage.py checks that every route of tests/golden/route_table.json has one).

Per case: the job reports the route the list recorded for it (so the case ran where it claims), the call goes through the product path
(`lib.deconvolution.richardson_lucy_MM`; an RLJob where params.fuse has to be set, which the wrapper does not expose), and u, the PSF and
the caller's PSF are compared with the pinned oracle -- scipy's complex64 FFT, the reference's own method: oracle/rl_mm_oracle.py for the
shipped loop, oracle/rl_ext_oracle.py for tv_mode 1 ... 3.  Gates are the suite's own: 1e-4 of max |ref| on u and the PSFs, per-outer
traces at rtol 2e-3 / atol 1e-7 (tests/test_gpu_small.py), identical iteration counts, stop flags and printed line counts; 1e-5 for
tv_mode 1 and the PAM kinds (tests/test_tv_mode.py).  Then the documented order-only and bit-identity claims, bit for bit, and the
rotation cache of the tile walk under concurrent jobs of different geometries."""
import contextlib
import io
import threading

import numpy as np
import pytest

import rl_ext_oracle as ext
import rl_mm_oracle as orc
import route_cases as rc

pytestmark = pytest.mark.gpu

TOL = 1e-4
TV_TOL = 1e-5
FLAT_TOL = 5e-3      # flat frames only: the residual is pure rounding noise, amplified by lambd on both sides (scripts/dbg/fuzz_runs.py)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def _args(c):
    return (*c.win, 1e9, c.M, c.N, 3, c.MK, c.iters, 1e-3, c.lambd)


def run_device(c, image, u0, psf0):
    """(u, psf_local, psf_caller, image after the call, stats, printed lines or None, route tuple) of the case on the device"""
    from lib import _native as nv
    from lib import deconvolution as dc
    with rc.switches_set(c):
        if c.fuse:
            job = nv.RLJob(c.M, c.N, c.MK)
            try:
                job.upload(image, u0, psf0)
                p = rc.params_of(nv, c)
                route = rc.route_tuple(job.describe(p))
                st = job.run(p)
                u, psf, psf_caller = job.download()
            finally:
                job.close()
            return u, psf, psf_caller, image, st, None, route
        job = dc._get_job(c.M, c.N, c.MK)
        route = rc.route_tuple(job.describe(rc.params_of(nv, c)))
        img, u, psf = image.copy(), u0.copy(), psf0.copy()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            dc.richardson_lucy_MM(img, u, psf, *_args(c), blind=c.blind, correlation=bool(c.correlation), tv_mode=c.tv_mode, conv=c.conv,
                                  flags=c.flags)
        st = dc.richardson_lucy_MM.last
        psf_local = job.download()[1]
        return u, psf_local, psf, img, st, len(buf.getvalue().splitlines()), route


def run_oracle(c, image, u0, psf0, direct=False, margins=None):
    """(u, psf_local, psf_caller, image after the call, Trace); `margins` (PAM kinds): a list that collects the arg-max margins of u"""
    img, u, psf = image.copy(), u0.copy(), psf0.copy()
    tr = orc.Trace()
    with np.errstate(all="ignore"):
        if c.tv_mode == 0:
            orc.richardson_lucy_MM(img, u, psf, *_args(c), blind=c.blind, correlation=bool(c.correlation), trace=tr, quiet=True,
                                   conv="direct" if direct else "scipy")
        elif c.tv_mode == 1:
            ext.richardson_lucy_MM_tv(img, u, psf, *_args(c), blind=c.blind, correlation=bool(c.correlation), conv="direct" if direct else "scipy", trace=tr)
        else:
            ext.richardson_lucy_PAM(img, u, psf, *_args(c), blind=c.blind, correlation=bool(c.correlation), collaborative=c.tv_mode == 3,
                                    conv="direct" if direct else "scipy", trace=tr, margins=margins)
    return u, tr.psf_final, psf, img, tr


def _pam_check(c, u, u_dir, margins, image, u0, psf0):
    """u of a PAM case against the direct-sum oracle, by the criteria of tests/test_tv_mode.py.

    The TV term of a nearly flat pixel (|grad u| within a few hundred epsilon; epsilon = 1e-6 non-blind) turns on any rounding difference of
    two correct convolutions, and the collaborative term's arg-max channel flips on 1e-7 differences at near-tie pixels.  So: the 1e-5 gate
    (the collaborative kind: its bulk at 1e-5, outliers by count and size) -- or, where the trajectory is not comparable at that level, the
    device no further from either oracle form (float64 direct sums, complex64 FFT) than 3 x their distance from each other, with that
    distance itself above 1e-5.  Collaborative outliers must in every case sit at or next to a pixel whose arg-max margin in the oracle's own
    trajectory came within the size of the deviations (the chain test of tests/test_tv_mode.py).  Returns (error against the direct form,
    how it passed)."""
    d = np.abs(u.astype(np.float64) - u_dir) / np.abs(u_dir).max()
    e_dir = float(d.max())
    if c.tv_mode == 3:
        out = d.max(axis=2) > 1e-5
        if out.any():
            from scipy.ndimage import binary_dilation
            m = np.min(np.stack(margins), axis=0) / np.abs(u_dir).max()
            chain = binary_dilation(m < 2.0 * e_dir, iterations=2)
            assert (out & chain).sum() == out.sum(), (c.id, "an outlier that no near-tie explains: not an arg-max flip")
        if np.mean(d > 1e-5) < 2e-3 and e_dir < 5e-3:
            return e_dir, "gate"
    elif e_dir <= TV_TOL:
        return e_dir, "gate"
    u_fft = run_oracle(c, image, u0, psf0)[0]
    o, e_fft = _rel(u_fft, u_dir), _rel(u, u_fft)
    print("   %s: device vs direct oracle %.2e | vs FFT oracle %.2e | FFT oracle vs direct oracle %.2e" % (c.id, e_dir, e_fft, o))
    assert o > TV_TOL and e_dir < 3.0 * o + 1e-6 and e_fft < 3.0 * o + 1e-6, (c.id, e_dir, e_fft, o)
    return e_dir, "spread"


def check_case(c, route_char=None):
    image, u0, psf0 = rc.make_data(c)
    u, psf, psf_caller, img, st, nlines, route = run_device(c, image, u0, psf0)
    if route_char is not None:
        assert rc.legend()[route] == route_char, (c.id, route, route_char)
    assert np.isfinite(u).all() and np.isfinite(psf).all() and np.isfinite(psf_caller).all(), c.id      # finite inputs: never NaN
    margins = [] if c.tv_mode >= 2 else None
    # the PAM kinds against the float64 direct-sum form of their oracle, as tests/test_tv_mode.py compares them (see _pam_check)
    oracle = "direct" if c.tv_mode >= 2 else "fft"
    assert oracle == "fft" or c.M * c.N * c.MK ** 2 <= rc.DIRECT_CAP, c.id
    u_r, psf_r, psfc_r, img_r, tr = run_oracle(c, image, u0, psf0, direct=oracle == "direct", margins=margins)
    if c.tv_mode == 0 and not (np.isfinite(u_r).all() and np.isfinite(psf_r).all()):
        # the oracle's FFT noise met an exact zero inside a black region: compare with the float64 direct-sum oracle and its 0/0 rule
        assert c.M * c.N * c.MK ** 2 <= rc.DIRECT_CAP, c.id
        u_r, psf_r, psfc_r, img_r, tr = run_oracle(c, image, u0, psf0, direct=True)
        oracle = "direct"
    flat = c.variant[0] == "flat"
    gate = FLAT_TOL if flat else (TOL if c.tv_mode == 0 else TV_TOL)
    eu, ep, epc = _rel(u, u_r), _rel(psf, psf_r), _rel(psf_caller, psfc_r)
    r = route_char or rc.legend()[route]
    print("route %s %-60s oracle %-6s u %.2e psf %.2e caller psf %.2e (gate %.0e)" % (r, c.id, oracle, eu, ep, epc, gate))
    assert st.iterations_done == tr.iterations and bool(st.stopped) == bool(tr.stopped), (c.id, st.iterations_done, tr.iterations, st.stopped, tr.stopped)
    if c.tv_mode >= 2:
        how = _pam_check(c, u, u_r, margins, image, u0, psf0)[1]
        print("   %s: PAM u passed by %s" % (c.id, how))
    else:
        assert eu <= gate, (c.id, eu)
    if c.blind:
        assert ep <= gate and epc <= gate, (c.id, ep, epc)
    if c.tv_mode == 1:
        assert _rel(img, img_r) <= gate, c.id
    if c.tv_mode == 0:
        if nlines is not None:
            assert nlines == len(tr.log.getvalue().splitlines()), c.id
        if not flat:
            n = st.trace_len
            names = ["Hu", "dof_min", "dof_max"]
            # M_r (whiteness of the residual in the window): not where the oracle's residual is its FFT's rounding noise over a black band
            # (the device's is exactly 0 there), nor on frames narrower than the PSF (a few residual pixels)
            if c.variant[0] not in ("black_top", "black_left", "black_bottom") and min(c.M, c.N) >= c.MK:
                names.append("M_r")
            names.append("varu")
            for name in names:
                got, ref = np.array(getattr(st, "trace_" + name)[:n], np.float64), np.array(getattr(tr, name), np.float64)
                assert got.shape == ref.shape and np.allclose(got, ref, rtol=2e-3, atol=1e-7, equal_nan=True), (c.id, name, got, ref)


@pytest.mark.parametrize("c", [c for c in rc.cases() if c.id not in rc.EXCLUDED], ids=lambda c: c.id)
def test_case_against_the_oracle(c):
    check_case(c, rc.routes()[c.id])


@pytest.mark.parametrize("conv", [1, 2, 3])
def test_random_edge_shapes_per_forced_family(conv):
    """Seeded hypothesis top-up: 8 whole calls per forced family over the same edge-biased shapes and PSF sizes."""
    from hypothesis import HealthCheck, given, settings, strategies as st
    sizes = {1: [3, 7, 15, 17, 23, 31, 33, 39, 49, 51, 63, 65, 71], 2: [3, 5, 9, 13, 15, 17, 21, 23, 25, 31, 33, 37, 39, 49],
             3: [3, 9, 15, 21, 25, 27, 31, 41, 45, 63, 85, 87]}[conv]

    def side(MK, d):
        kind = d.draw(st.sampled_from(["tile64", "fft", "small"]))
        k = d.draw(st.integers(1, 3))
        e = d.draw(st.sampled_from([-1, 0, 1]))
        if kind == "tile64":
            s = 64 * k + e
        elif kind == "fft":
            s = k * rc.tile_valid(MK, conv == 3 and MK <= rc.CONV2_MAX_K) + e
        else:
            s = d.draw(st.integers(1, 48))
        return max(1, min(s, 300))

    @settings(max_examples=8, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(st.sampled_from(sizes), st.booleans(), st.integers(0, 10 ** 6), st.sampled_from(["plain", "scaled"]), st.data())
    def check(MK, blind, seed, variant, d):
        M, N = side(MK, d), side(MK, d)
        rng = np.random.default_rng(seed)
        win = rc._window(rng, M, N, MK)
        var = ("scaled", float(10.0 ** int(rng.integers(-6, 5)))) if variant == "scaled" else ("plain",)
        c = rc.Case("hyp-%dx%d-k%d" % (M, N, MK), M, N, MK, blind, conv=conv, win=win, variant=var, seed=seed)
        check_case(c)

    check()


# ---- order-only and bit-identity claims, bit for bit -------------------------------------------------------------------------------------
def _exact(c, **over):
    image, u0, psf0 = rc.make_data(c)
    from lib import _native as nv
    job = nv.RLJob(c.M, c.N, c.MK)
    try:
        job.upload(image, u0, psf0)
        with rc.switches_set(c):
            p = rc.params_of(nv, c)
            for k, v in over.items():
                setattr(p, k, v)
            route = rc.route_tuple(job.describe(p))
            st = job.run(p)
        u, psf, psfc = job.download()
        n = st.trace_len
        tr = [np.array(getattr(st, "trace_" + f)[:n]) for f in ("M_r", "Hu", "varu", "dof_min", "dof_max")]
        return route, [u, psf, psfc] + tr, (st.iterations_done, st.stopped)
    finally:
        job.close()


def _same(a, b):
    assert a[2] == b[2]
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("conv,MK,blind,path", [(1, 9, True, 0), (1, 13, True, 0), (1, 15, False, 0), (1, 21, False, 0), (1, 31, False, 0),
                                                 (0, 13, True, 1), (0, 23, False, 1)])
def test_fuse_is_bit_identical_on_the_fp32_kernels(conv, MK, blind, path):
    """include/ics_hip.h params.fuse: the update fused into the next convolution (u ping-pong).  The fused kernel is an fp32 one (do_conv,
    mode 2), so on the fp32 routes -- params.conv = 1, and ICS_CONV_AUTO sent there by ICS_CONV_PATH=vector -- the results are bit-identical.
    (The fused A11 + A13 kernel is off in both runs: fuse = 1 never takes it, and it is another summation order of the PSF gradient.)"""
    c = rc.Case("fuse", 200, 190, MK, blind, conv=conv, flags=rc.FLAG_NO_FUSED_GRADK, win=(10, 180, 20, 170), seed=MK,
                switches=(("conv_path", path), ("small_iter", 0)))
    a, b = _exact(c, fuse=0), _exact(c, fuse=1)
    assert a[0] == b[0] and a[0][1] == 0, (a[0], b[0])
    _same(a, b)


@pytest.mark.parametrize("conv,MK,blind", [(2, 9, True), (2, 21, False), (0, 17, True), (0, 13, False)])
def test_fuse_on_the_matrix_cores_runs_the_synthesis_on_the_fp32_kernels(conv, MK, blind):
    """On a matrix-core route fuse = 1 is not bit-identical, by construction: the fused update + synthesis (do_conv, mode 2) exists on the
    fp32 kernels only, so A1 of every inner iteration after the first of an outer one takes fp32 products instead of fp16-split ones.  Pinned
    here: each form is deterministic (two runs bit for bit), the two differ, and only by the rounding of the products (<= 1e-5)."""
    c = rc.Case("fuse", 200, 190, MK, blind, conv=conv, flags=rc.FLAG_NO_FUSED_GRADK, win=(10, 180, 20, 170), seed=MK,
                switches=(("small_iter", 0),))
    a, a2, b, b2 = _exact(c, fuse=0), _exact(c, fuse=0), _exact(c, fuse=1), _exact(c, fuse=1)
    assert a[0] == b[0] and a[0][1] == 1, (a[0], b[0])
    _same(a, a2)
    _same(b, b2)
    assert not np.array_equal(a[1][0], b[1][0])
    print("fuse 1 vs 0, conv %d %d x %d blind=%d: u %.2e psf %.2e" % (conv, MK, MK, blind, _rel(b[1][0], a[1][0]), _rel(b[1][1], a[1][1])))
    assert a[2] == b[2] and _rel(b[1][0], a[1][0]) <= 1e-5 and _rel(b[1][1], a[1][1]) <= 1e-5


@pytest.mark.parametrize("conv,MK,blind", [(1, 31, False), (2, 15, True), (3, 31, True), (0, 21, True)])
def test_varu_of_a_window_that_ends_inside_the_pad_follows_numpy(conv, MK, blind):
    """pyx:600 slices u[top + pad:bottom - pad, left + pad:right - pad]: with bottom < pad (right < pad) the stop is negative and numpy counts
    it from the end of the u-frame, so the reference's varu is that of a non-empty window -- not NaN.  The device follows it (make_win)."""
    M, N = 120, 110
    c = rc.Case("varu", M, N, MK, blind, conv=conv, win=(2, MK // 2 - 3, 4, MK // 2 - 1), seed=7)
    image, u0, psf0 = rc.make_data(c)
    st = run_device(c, image, u0, psf0)[4]
    tr = run_oracle(c, image, u0, psf0)[4]
    got, ref = np.array(st.trace_varu[:st.trace_len], np.float64), np.array(tr.varu, np.float64)
    print("varu, window ending inside the pad, conv %d: device %s oracle %s" % (conv, got, ref))
    assert np.isfinite(ref).all() and got.shape == ref.shape and np.allclose(got, ref, rtol=2e-3, atol=1e-7)


@pytest.mark.parametrize("blind,wgs", [(True, 0), (False, 0), (True, 5), (False, 3)])
def test_tile_walk_rotation_is_order_only(blind, wgs):
    """ics_launch_conv2_fft: where the walk of mode 2's units starts changes the order only."""
    base = rc.Case("rot", 380, 350, 15, blind, conv=3, win=(5, 370, 10, 340), seed=3, switches=(("max_wgs", wgs),))
    rot0 = dataclasses_replace(base, switches=(("fft_rot", 0), ("max_wgs", wgs)))
    a, b = _exact(base), _exact(rot0)
    assert a[0] == b[0] and a[0][0] == 5
    _same(a, b)


@pytest.mark.parametrize("conv,MK,blind,route", [(2, 9, True, "8"), (2, 17, False, "c"), (2, 19, True, "d")])
def test_image_copy_in_accumulator_order_is_bit_identical(conv, MK, blind, route):
    """planar_image = 0: the epilogues read the HWC image instead of its accumulator-order copy (ics_image_acc.h): the same values."""
    c = rc.Case("acc", 200, 190, MK, blind, conv=conv, win=(10, 180, 20, 170), seed=MK)
    off = dataclasses_replace(c, switches=(("planar_image", 0),))
    a, b = _exact(c), _exact(off)
    leg = rc.legend()
    assert leg[a[0]] == route and a[0][4] == 1 and b[0][4] == 0
    _same(a, b)


def dataclasses_replace(c, **kw):
    import dataclasses
    return dataclasses.replace(c, **kw)


# ---- the rotation cache of the tile walk under concurrent jobs ----------------------------------------------------------------------------
def test_concurrent_jobs_of_different_geometries_on_the_tiles():
    """Two host threads, each with its own job on the transform tiles (conv = 3, 15 x 15: mode 2 runs) and very different unit counts, run
    their calls concurrently, as lib/banded.py's band jobs do: every result is bit-identical to the same calls made one after the other."""
    from lib import _native as nv
    shapes = [(900, 900), (140, 140)]
    calls = 4
    setup = []
    for i, (M, N) in enumerate(shapes):
        c = rc.Case("conc", M, N, 15, False, conv=3, win=(10, M - 10, 10, N - 10), seed=40 + i)
        image, u0, psf0 = rc.make_data(c)
        job = nv.RLJob(M, N, 15)
        setup.append((c, job, image, u0, psf0))

    def one(k):
        c, job, image, u0, psf0 = setup[k]
        job.upload(image, u0, psf0)
        p = rc.params_of(nv, c)
        assert job.describe(p).conv_family == 5
        st = job.run(p)
        return job.download()[0], (st.iterations_done, st.stopped)

    try:
        seq = [[one(k) for _ in range(calls)] for k in range(len(setup))]
        got = [[None] * calls for _ in setup]
        errors = []
        start = threading.Barrier(len(setup))

        def worker(k):
            try:
                start.wait()
                for i in range(calls):
                    got[k][i] = one(k)
            except BaseException as e:     # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=worker, args=(k,)) for k in range(len(setup))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        for k in range(len(setup)):
            for i in range(calls):
                assert got[k][i][1] == seq[k][i][1]
                assert np.array_equal(got[k][i][0], seq[k][i][0]), (shapes[k], i)
    finally:
        for s in setup:
            s[1].close()
