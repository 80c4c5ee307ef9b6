"""GPU: the stop-test statistics (csrc/ics_stats.hip: M_r, Hu, varu) of ICS_STAGE_STATS alone, on residuals the test writes itself,
against the float64 reference of tests/stats_ref.py -- on fields whose M_r depends on where every lag is read (a pair of impulses per
channel at the extreme lags, pairs at the first lags that must not be read, a comb of unequal impulses), on every transform form the
two paths have: P = 4 .. 8192 with C = 4, 2 and 1 lines per workgroup, idle lanes, the configured-LDS sizes, even and odd sides, one
degenerate axis, windows flush with two corners of the frame; the long-line path with Py at its floor of 64, C = 2, four blocks along
x, even and odd sides.

Gates: 4 x the error of the float32 restatement of the same operations (stats_ref.F32_RESTATEMENT_ERROR, measured on the CPU without the
code under test), never above the gates of tests/test_gpu_stages.py (2e-4 for M_r, 1e-5 for Hu and varu).  tests/test_stats_ref.py
asserts that each gate lies 100 x below what one lag, weight or scale slip does to M_r on the same window.

Measured on an MI355X, worst error / gate of M_r per form: P = 2 0.25, P = 4 .. 8 0.41, P = 16 .. 64 0.39, P = 128 / 256 0.11, one
degenerate axis (P = 1024) 0.25, P = 1024 0.33, P = 2048 0.39, P = 4096 0.25, P = 8192 0.60, the corner windows 0.37; long lines: Py = 64
0.25, Py = 2048 (C = 2) 0.19, Px = 32768 0.25, Py = 16384 0.32 (even sides) and 0.10 (odd); the large-mean window 0.52 of the 2e-4
cap.  Hu and varu are 0.25 everywhere: the device gives the restatement's value bit for bit."""
import functools
import gc

import numpy as np
import pytest

import stats_ref as sr

pytestmark = pytest.mark.gpu
BY_ID = {c.id: c for c in sr.CASES + sr.BIG_CASES}
NAMES = ("M_r", "Hu", "varu")


@functools.lru_cache(maxsize=None)
def expected(case_id, gen):
    """the float64 reference of one case and field, computed once"""
    c = BY_ID[case_id]
    return sr.reference(sr.field(gen, c.H, c.W, sr.SEED), c.u_window(c.u_frame()))


def new_job(M, N, u):
    from lib import _native as nv
    job = nv.RLJob(M, N, sr.MK)
    job.upload(np.zeros((M, N, 3), np.float32), u, np.full((sr.MK, sr.MK, 3), 1.0 / sr.MK ** 2, np.float32))
    return job


def stats(job, win):
    """ICS_STAGE_STATS alone: the residual is whatever BUF_ERROR holds"""
    from lib import _native as nv
    job.stage(nv.STAGE_STATS, job.params(*win, 1e9, 1, 1e-3, 10000.0, blind=False))
    sc = job.scalars()
    return tuple(sc[n] for n in NAMES)


def check(label, got, ref, gates):
    """every statistic within its gate of the reference (NaN where the reference is NaN); returns the ratios error / gate"""
    ratios = []
    for name, g, r, gate in zip(NAMES, got, ref, gates):
        if r != r:
            assert g != g, (label, name, g)
            continue
        err = abs(g - r) / abs(r)
        ratios.append(err / gate)
        print("%s %s: error %.3e, gate %.3e, ratio %.3f" % (label, name, err, gate, err / gate))
        assert err <= gate, (label, name, g, r, err, gate)
    return ratios


def run_case(c, gens):
    from lib import _native as nv
    job = new_job(c.M, c.N, c.u_frame())
    try:
        for gen in gens:
            e = c.error_frame(gen)
            job.write(nv.BUF_ERROR, e)
            got = stats(job, c.win)
            if c.M * c.N <= 1 << 16:
                assert np.array_equal(job.read(nv.BUF_ERROR), e)        # the stage read the residual and left it alone
            check("%s %s %s" % (c.klass, c, gen), got, expected(c.id, gen), sr.gates(c.id))
    finally:
        job.close()


@pytest.mark.parametrize("c", sr.CASES, ids=repr)
def test_small_path_windows(c):
    run_case(c, c.gens)


@pytest.mark.parametrize("gen", sr.ALL3)
@pytest.mark.parametrize("c", sr.BIG_CASES, ids=repr)
def test_long_line_windows(c, gen):
    run_case(c, (gen,))


def test_a_grey_one_by_one_window_gives_nan_as_the_reference_does():
    """three equal values: deviation 0, (e - mean) / std is 0 / 0 in pyx:627 and on the device; Hu is their mean square.  (With three
    different values the window has a finite M_r: the P2 case of stats_ref.CASES.)"""
    from lib import _native as nv
    M, N, grey = 20, 24, np.float32(0.37)
    e = np.array(sr.rough(M, N, sr.SEED))
    e[5, 9] = grey
    assert np.isnan(sr.reference(e[5:6, 9:10], e[:0])[0])
    job = new_job(M, N, np.zeros((M + 2 * sr.PAD, N + 2 * sr.PAD, 3), np.float32))
    try:
        job.write(nv.BUF_ERROR, e)
        M_r, Hu, varu = stats(job, (5, 6, 9, 10))
        print("grey 1 x 1: M_r %r, Hu %r, varu %r" % (M_r, Hu, varu))
        assert M_r != M_r and varu != varu and abs(Hu - float(grey) ** 2) <= sr.HU_CAP * float(grey) ** 2
    finally:
        job.close()


def test_moments_of_a_window_with_a_large_mean():
    """k_mom1 / k_mom2 on 700 x 701 x 3 values: a second trip of the batched loop with a count that is no multiple of the batch, a
    residual around 1000 and a u around 250, where (x - mean) cancels the leading digits"""
    from lib import _native as nv
    c = sr.MOMENTS
    e, u = sr.moments_frames()
    ref = sr.reference(e[c.win[0]:c.win[1], c.win[2]:c.win[3]], c.u_window(u))
    job = new_job(c.M, c.N, u)
    try:
        job.write(nv.BUF_ERROR, e)
        check("moments %s" % c, stats(job, c.win), ref, sr.gates(c.id))
    finally:
        job.close()


def test_sequence_of_windows_on_one_job_and_a_nan_between_clean_calls():
    """window A (P = 256), B (P = 64), A again: the window cache rebuilds tables, weights and scratch each time.  Then A with one NaN
    inside gives NaN, and the call after it is clean: the NaN key and the accumulators are re-armed"""
    from lib import _native as nv
    A, B = BY_ID["71x100@20,20"], BY_ID["16x17"]
    assert A.sizes[0] == 256 and B.sizes[0] == 64 and B.win[1] <= A.win[0]       # B lies above A in A's frame: one residual holds both
    e = A.error_frame("pairs")
    e[B.win[0]:B.win[1], B.win[2]:B.win[3]] = sr.field("pairs", B.H, B.W, sr.SEED)
    u = A.u_frame()
    u[B.top + sr.PAD:B.win[1] - sr.PAD, B.left + sr.PAD:B.win[3] - sr.PAD] = B.u_window(B.u_frame())
    job = new_job(A.M, A.N, u)
    try:
        job.write(nv.BUF_ERROR, e)
        for step, c in enumerate((A, B, A)):
            check("sequence step %d %s" % (step, c), stats(job, c.win), expected(c.id, "pairs"), sr.gates(c.id))
        bad = e.copy()
        bad[A.top + 30, A.left + 40, 1] = np.nan
        job.write(nv.BUF_ERROR, bad)
        M_r, Hu, varu = stats(job, A.win)
        assert M_r != M_r and Hu != Hu, (M_r, Hu)
        assert abs(varu - expected(A.id, "pairs")[2]) <= sr.HU_CAP * varu
        job.write(nv.BUF_ERROR, e)
        check("sequence after NaN %s" % A, stats(job, A.win), expected(A.id, "pairs"), sr.gates(A.id))
        check("sequence after NaN %s" % B, stats(job, B.win), expected(B.id, "pairs"), sr.gates(B.id))
    finally:
        job.close()


@pytest.mark.parametrize("case_id", ["513x64", "513x4200"], ids=["P2048-C2", "long-line-Py2048-C2"])
def test_on_poisoned_red_zoned_pool_blocks(debug_switch, case_id):
    """pool check mode (csrc/ics_pool.h): the spectrum scratch is filled with 0xFF (NaN) when the job takes it and its red zone verified when
    it goes back.  k_fft_cols / k_big_cols write back only the rows the last pass reads: a read of a row nobody wrote would turn M_r
    into NaN, a store past the scratch would be counted"""
    from lib import _native as nv
    c = BY_ID[case_id]
    e, u, ref, gates = c.error_frame("pairs"), c.u_frame(), expected(case_id, "pairs"), sr.gates(case_id)

    def run():
        job = new_job(c.M, c.N, u)
        try:
            job.write(nv.BUF_ERROR, e)
            return stats(job, c.win)
        finally:
            job.close()

    clean = run()
    gc.collect()
    nv.debug_set("pool_overruns", 0)
    debug_switch("pool_check", 0xFF)
    poisoned = run()
    gc.collect()
    debug_switch("pool_check", -1)
    gc.collect()
    nv.Context.get().conv2d_symm(np.zeros((2, 2)), np.ones((1, 1)))     # returns the context's last check-mode scratch block (tests/test_gpu_pool_check.py)
    assert nv.debug_set("pool_overruns", 0) == 0
    check("clean %s" % c, clean, ref, gates)
    check("poisoned %s" % c, poisoned, ref, gates)
    for name, a, b, gate in zip(NAMES, poisoned, clean, gates):
        assert abs(a - b) <= gate * abs(b), (name, a, b)
