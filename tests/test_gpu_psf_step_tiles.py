"""Blind runs on the transform tiles step the PSF and build both weight spectra in ONE launch behind k_gradk_fft_reduce (k_psf_spectra,
csrc/ics_conv_fft.hip; switch fft_psf1 / ICS_FFT_PSF1).  The pair it replaces -- k_psf, k_fft_spectrum -- stays behind the switch and
behind the stage API, and everything here is held against it BIT FOR BIT:

  * one outer iteration, switch on / switch off / the same iteration driven stage by stage (the old kernels), from 9 x 9 to 45 x 45:
    both instances of the kernel, and 25 / 27, where mode 2 of the tiles ends;
  * few and many blocks of the gradient in front of it: 3 and 6 workgroups, and 255 on a 1500^2 frame;
  * correlation = 1 (the `frozen` / psf_caller semantics), the undo of the overlapped loop across the PSF buffer exchange, and a
    matrix-core run right after a tile run on the same job (the weight tables the tile loop no longer packs).
"""
import numpy as np
import pytest

import psf_gradient_ref as pg
import rl_mm_oracle as orc

pytestmark = pytest.mark.gpu

STEP, LAMBD = 1e-3, 10000.0
_cases = {}


def _case(M, N, MK):
    """image, u0, psf0 of a blind problem; computed once per shape and never written to"""
    key = (M, N, MK)
    if key not in _cases:
        rng = np.random.default_rng(M + 7 * N + 31 * MK)
        if M * N <= 200000:
            case = orc.synth_case(M, N, MK, seed=MK + M, blind=True, per_channel_psf=True)
            image, u0 = case["image"], case["u0"]
        else:   # (large frames: no CPU convolution -- a smooth random picture, u0 = its edge-padded copy)
            small = rng.random((M // 8 + 2, N // 8 + 2, 3), dtype=np.float32)
            image = np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32))[:M, :N] * 0.8 + 0.1 * rng.random((M, N, 3), dtype=np.float32))
            pad = MK // 2
            u0 = np.ascontiguousarray(np.pad(image, ((pad, pad), (pad, pad), (0, 0)), mode="edge"))
        psf = pg.asymmetric_psf(MK, rng)   # no symmetry: flips show
        for a in (image, u0, psf):
            a.setflags(write=False)
        _cases[key] = (image, u0, psf)
    return _cases[key]


def _job(M, N, MK):
    from lib import _native as nv
    image, u0, psf = _case(M, N, MK)
    job = nv.RLJob(M, N, MK)
    job.upload(image, u0, psf)
    return job


def _params(job, iterations, conv, correlation=0):
    win = orc.default_window(job.M, job.N, job.MK)
    return job.params(*win, 1e9, iterations, STEP, LAMBD, blind=True, correlation=correlation, conv=conv)


def _state(job):
    from lib import _native as nv
    u, psf, caller = job.download()
    return {"u": u, "psf": psf, "psf_caller": caller, "gradk": job.read(nv.BUF_GRADK), "dtpsf": np.float32(job.scalars()["dtpsf"])}


def _same(a, b, keys=("u", "psf", "psf_caller", "gradk", "dtpsf"), what=""):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), "%s: %s differs" % (what, k)


def _run(M, N, MK, psf1, debug_switch, iterations=1, conv=None, correlation=0, progress=None):
    from lib import _native as nv
    debug_switch("fft_psf1", psf1)
    job = _job(M, N, MK)
    st = job.run(_params(job, iterations, nv.CONV_FFT if conv is None else conv, correlation), progress=progress)
    return job, st


# (31 and 33: the last size of the kernel's three-values-a-thread instance and the first of the other)
FRAMES = [(200, 180, 15), (150, 130, 9), (260, 300, 25), (260, 300, 27), (300, 300, 45), (150, 140, 31), (150, 140, 33)]


@pytest.mark.parametrize("M,N,MK", FRAMES)
def test_one_outer_iteration_on_off_and_stage_by_stage(M, N, MK, debug_switch):
    from lib import _native as nv
    out = {}
    for psf1 in (1, 0):
        job, st = _run(M, N, MK, psf1, debug_switch)
        assert st.iterations_done == 1 and not st.has_nan
        out[psf1] = _state(job)
        job.close()
    assert np.abs(out[1]["psf"] - _case(M, N, MK)[2]).max() > 0
    _same(out[1], out[0], what="switch on / off")
    # the same outer iteration with A1 and A3 as two kernels (what the stages run), switch on, against the iteration stage by stage:
    # majorise, then five times residual, back-projection, update, A11 + A13, PSF step -- the stage API keeps k_gradk_fft_reduce, k_psf
    # and k_fft_spectrum
    debug_switch("fft_conv2", 0)
    job, _ = _run(M, N, MK, 1, debug_switch)
    run2 = _state(job)
    job.close()
    job = _job(M, N, MK)
    p = _params(job, 1, nv.CONV_FFT)
    job.stage(nv.STAGE_MAJORIZE, p)
    for _ in range(5):
        for stage in (nv.STAGE_SYNTH_RESIDUAL, nv.STAGE_BACKPROJECT, nv.STAGE_UPDATE, nv.STAGE_SYNTH_GRADK, nv.STAGE_PSF_UPDATE):
            job.stage(stage, p)
    staged = _state(job)
    job.close()
    _same(run2, staged, what="run / stages")


@pytest.mark.parametrize("M,N,MK,max_wgs", [(200, 180, 15, 3), (200, 180, 15, 6), (1500, 1500, 15, 0)])
def test_block_counts_of_the_gradient_in_front(M, N, MK, max_wgs, debug_switch, ctx):
    if max_wgs:
        debug_switch("max_wgs", max_wgs)
    else:
        assert ctx.compute_units >= 255      # 170 tiles x 3 channels on one workgroup per CU: 255 blocks on an MI355X
    out = {}
    for psf1 in (1, 0):
        job, st = _run(M, N, MK, psf1, debug_switch)
        out[psf1] = _state(job)
        job.close()
    assert np.abs(out[1]["gradk"]).max() > 0
    _same(out[1], out[0], keys=("gradk", "psf", "psf_caller", "dtpsf"), what="%d workgroups" % max_wgs)


def test_correlation_freezes_the_callers_psf_as_before(debug_switch):
    out = {}
    for psf1 in (1, 0):
        job, st = _run(200, 180, 15, psf1, debug_switch, iterations=2, correlation=1)
        assert st.iterations_done == 2
        out[psf1] = _state(job)
        job.close()
    assert not np.array_equal(out[1]["psf"], out[1]["psf_caller"])       # (the caller's array kept the first raw step, pyx:585)
    assert np.array_equal(out[1]["psf"][..., 0], out[1]["psf"][..., 1])
    _same(out[1], out[0], what="correlation")


def test_undo_of_the_overlapped_loop_keeps_the_psf_buffers_straight(debug_switch):
    """the callback stops the run at outer iteration 2 while iteration 3 is queued: it is undone (the PSF comes back from psf_bak into
    whichever buffer is `psf` by then); a second run on the same job starts from there"""
    from lib import _native as nv
    out = {}
    for psf1 in (1, 0):
        job, st = _run(200, 180, 15, psf1, debug_switch, iterations=4, progress=lambda it, *rest: it == 2)
        assert st.iterations_done == 2 and st.stopped == 2
        first = _state(job)
        st = job.run(_params(job, 1, nv.CONV_FFT))
        assert st.iterations_done == 1
        out[psf1] = (first, _state(job))
        job.close()
    _same(out[1][0], out[0][0], keys=("u", "psf", "psf_caller"), what="after the undo")
    _same(out[1][1], out[0][1], what="second run")


def test_matrix_core_run_after_a_tile_run_repacks_its_tables(debug_switch):
    from lib import _native as nv
    M, N, MK = 200, 180, 15
    job, _ = _run(M, N, MK, 1, debug_switch)
    u1, psf1, _caller = job.download()
    assert np.abs(psf1 - _case(M, N, MK)[2]).max() > 0
    job.run(_params(job, 1, nv.CONV_MATRIX))
    after = _state(job)
    job.close()
    fresh = nv.RLJob(M, N, MK)
    fresh.upload(_case(M, N, MK)[0], u1, psf1)
    fresh.run(_params(fresh, 1, nv.CONV_MATRIX))
    want = _state(fresh)
    fresh.close()
    _same(after, want, what="matrix-core run after a tile run")
