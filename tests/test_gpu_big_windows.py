"""Stop-test statistics on windows with a side above 4096 px: the long-line path of csrc/ics_stats.hip (per-axis transforms of up
to 32768 points, lines above 8192 points split into in-LDS blocks).  Each window here was refused with ICS_ENOSUP before; the gates
are those of tests/test_gpu_stages.py::test_window_statistics_and_whiteness_metric."""
import contextlib
import io

import numpy as np
import pytest

import rl_mm_oracle as orc
from helpers import assert_log_matches, rel_err

pytestmark = pytest.mark.gpu


def stage_job(M, N, MK, seed):
    """a job holding a random u and image: the residual of ICS_STAGE_SYNTH_RESIDUAL is a rough, non-white field"""
    from lib import _native as nv
    rng = np.random.default_rng(seed)
    pad = MK // 2
    u = rng.random((M + 2 * pad, N + 2 * pad, 3), dtype=np.float32)
    image = rng.random((M, N, 3), dtype=np.float32)
    psf = np.full((MK, MK, 3), 1.0 / (MK * MK), np.float32)
    job = nv.RLJob(M, N, MK)
    job.upload(image, u, psf)
    return job


def stats_of(job, win, MK):
    from lib import _native as nv
    p = job.params(*win, 1e9, 1, 1e-3, 10000.0, blind=False)
    job.stage(nv.STAGE_SYNTH_RESIDUAL, p)
    job.stage(nv.STAGE_STATS, p)
    sc = job.scalars()
    return sc["M_r"], sc["Hu"], sc["varu"]


def check_against_oracle(job, win, MK, sc):
    from lib import _native as nv
    e, u = job.read(nv.BUF_ERROR), job.read(nv.BUF_U)
    top, bottom, left, right = win
    pad = MK // 2
    ew = e[top:bottom, left:right]
    M_r = orc.residual_whiteness(ew, orc.stop_weights(*win), orc._conv_scipy)
    # float64 sums: numpy's float32 norm of ~5e7 values drifts by ~3e-4, the device accumulates in double
    Hu = np.sum(ew.astype(np.float64) ** 2) / ((bottom - top) * (right - left) * 3)
    varu = np.std(u[top + pad:bottom - pad, left + pad:right - pad].astype(np.float64)) ** 2
    assert abs(sc[0] - M_r) / M_r < 2e-4, (sc[0], M_r)
    assert abs(sc[1] - Hu) / Hu < 1e-5
    assert abs(sc[2] - varu) / varu < 1e-5


# (frame M, N, window): Py x Px of the transforms in the comment
BIG = [
    pytest.param(4620, 360, (10, 4610, 15, 345), id="4600x330-Py16384-Px1024"),
    pytest.param(360, 4620, (15, 345, 10, 4610), id="330x4600-Py1024-Px16384"),
    pytest.param(4210, 4210, (5, 4205, 5, 4205), id="4200x4200-Py16384-Px16384"),
    pytest.param(8310, 220, (5, 8305, 10, 210), id="8300x200-Py32768-Px512"),
]


@pytest.mark.parametrize("M,N,win", BIG)
def test_big_window_statistics_against_the_oracle(M, N, win):
    MK = 3
    job = stage_job(M, N, MK, seed=M + N)
    try:
        check_against_oracle(job, win, MK, stats_of(job, win, MK))
    finally:
        job.close()


def test_job_reuse_big_small_big_window():
    """the window cache: big window (long-line path) -> small window (P x P path) -> big window again on one job"""
    M, N, MK = 4400, 300, 3
    big, small = (0, M, 0, N), (100, 400, 20, 280)
    job = stage_job(M, N, MK, seed=11)
    try:
        a = stats_of(job, big, MK)
        check_against_oracle(job, big, MK, a)
        b = stats_of(job, small, MK)
        check_against_oracle(job, small, MK, b)
        c = stats_of(job, big, MK)
        np.testing.assert_allclose(c, a, rtol=1e-6)
        assert stats_of(job, small, MK) == pytest.approx(b, rel=1e-6)
    finally:
        job.close()


def test_big_window_allocation_failure_leaves_the_job_usable(debug_switch):
    from lib import _native as nv
    M, N, MK = 4400, 300, 3
    big, small = (0, M, 0, N), (10, 200, 10, 200)
    job = stage_job(M, N, MK, seed=12)
    try:
        first = stats_of(job, big, MK)
        for nth in (1, 2, 3):
            stats_of(job, small, MK)                       # the cached key is the small window: the big one allocates again
            debug_switch("fail_window_alloc", nth)
            with pytest.raises(nv.NativeError) as ei:
                stats_of(job, big, MK)
            assert ei.value.code == nv.ICS_ENOMEM and "bytes" in str(ei.value)
            np.testing.assert_allclose(stats_of(job, big, MK), first, rtol=1e-6)
    finally:
        job.close()


@pytest.mark.parametrize("M,N", [(4300, 96), (96, 4300)])
def test_whole_frame_window_run_against_the_oracle(M, N):
    """ics_rl_run with the whole frame as the stats window (as tests/test_gpu_edges.py does on small frames), on frames with a side
    above 4096 px: the per-outer M_r, the printed lines and the stop decision of the oracle"""
    from lib import deconvolution as dc
    MK, iters = 5, 2
    case = orc.synth_case(M, N, MK, seed=M // 7 + N)
    win = (0, M, 0, N)
    args = (*win, 1e9, M, N, 3, MK, iters, 1e-3, 1e4)
    u_r, psf_r = case["u0"].copy(), case["psf0"].copy()
    tr = orc.Trace()
    ref_buf = io.StringIO()
    with contextlib.redirect_stdout(ref_buf):
        orc.richardson_lucy_MM(case["image"].copy(), u_r, psf_r, *args, blind=False, trace=tr)
    u, psf = case["u0"].copy(), case["psf0"].copy()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        dc.richardson_lucy_MM(case["image"].copy(), u, psf, *args, blind=False)
    st = dc.richardson_lucy_MM.last
    assert st.iterations_done == tr.iterations == iters and bool(st.stopped) == bool(tr.stopped)
    n = st.trace_len
    assert n == len(tr.M_r) == iters
    np.testing.assert_allclose(np.array(st.trace_M_r[:n]), np.array(tr.M_r), rtol=2e-4)
    assert rel_err(u, u_r) < 1e-4
    assert_log_matches(buf.getvalue(), ref_buf.getvalue(), 2e-4)


def test_deblur_module_mask_size_1201_host_and_resident_drivers_agree(capsys):
    """mask_size 1201 was refused before the first solver call (a cap of 1025 in the driver)"""
    import deconvolve as dv
    case = orc.synth_case(1300, 1310, 5, seed=8)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask_size=1201, display=False, iterations=2, pyramid=False, save=False)
    out_h, psf_h = dv.deblur_module(pic, "h", ".", 5, device_resident=False, **kw)
    log_h = capsys.readouterr().out
    out_d, psf_d = dv.deblur_module(pic, "d", ".", 5, device_resident=True, **kw)
    log_d = capsys.readouterr().out
    assert "Mask size : 1201 × 1201" in log_h
    assert out_d.shape == out_h.shape == (1300, 1310, 3)
    assert np.abs(psf_d - psf_h).max() < 1e-5
    assert np.abs(out_d - out_h).max() / 65535 < 2e-5, np.abs(out_d - out_h).max()
    strip = lambda t: [l for l in t.splitlines() if not l.startswith("'deblur_module'") and "sec" not in l]
    assert [l.split("=")[0] for l in strip(log_h)] == [l.split("=")[0] for l in strip(log_d)]
