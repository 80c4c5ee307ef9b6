"""A used job equals a fresh one, bit for bit (tests/reuse_cases.py: the run kinds, the shapes, the data, the table of what a job carries).

A fresh job is pinned to the oracle on every route (goldens, tests/test_gpu_route_matrix.py, the pool-check tests); "the state after a
sequence of calls on one job = the state of a fresh job after the last call alone, every bit" carries that pin over to every sequence.  The
state of a job is `_state` of tests/test_gpu_maxg_select.py -- u, both PSFs, the scalars, the five traces, the counters, the six reduction keys
of every inner iteration -- compared with its `_same`.

  P0  two fresh jobs give the same state: the premise (every kind, 1, 2 and 3 outer iterations).  No exception was needed: no field of no kind is left out.
  P1  upload(D_a), run A, upload(D_b), run B = fresh upload(D_b), run B: every ordered pair of kinds of a shape, run A with 1, 2, 3 outer iterations
      cycling over the pairs and with each of them in front of three fixed Bs (all three phases of the u / ut / u2 rotation, both parities of the
      PSF swap); run A ended by the progress callback under overlap = 2 (undo) and run A with correlation = 1 (the frozen flag) in front of every B.
      What P1 found: the scalars of a non-blind run behind a blind one kept the blind run's dtpsf (a fresh job reports 0) -- every blind A in front of
      every non-blind B, nothing else.  ics_rl_run now zeroes the scalars with the rest of the job's small state (k_run_reset).
  P2  every way to change the image invalidates every copy derived from it: write, write_rows and copy_rows of some rows, upload_img from windows of
      larger device images, the image-stepping update of tv_mode 1; download_img; the drop-in calls of lib/deconvolution.py on a cached job.
  P3  single stages on a used job, on every convolution family, behind an upload and behind ics_rl_write of the frames and the PSF.
  P4  what ics_rl_read returns after a run (include/ics_hip.h ICS_BUF_*).
"""
import contextlib
import io

import numpy as np
import pytest

import reuse_cases as ru
from test_gpu_maxg_select import _get, _same, _state

pytestmark = pytest.mark.gpu

_fresh = {}


def _id(k):
    return k.id


def _new_job(shape):
    from lib import _native as nv
    return nv.RLJob(*ru.SHAPES[shape])


def _upload(job, d, k):
    job.upload(d["image"], d["u"], ru.psf_of(d, k))


def _run(job, k, n, progress=None):
    from lib import _native as nv
    with ru.switches_set(k):
        st = job.run(ru.params_of(nv, k, n), progress=progress)
        return _state(job, st)


def _eq(a, b, what):
    nan = bool(a["iterations"][2] or b["iterations"][2])
    _same(a, b, what, any_nan_in_statistics=nan)


def _fresh_run(k, n, image=None, u=None, psf=None):
    d = ru.data(k.shape)["b"]
    job = _new_job(k.shape)
    job.upload(d["image"] if image is None else image, d["u"] if u is None else u, ru.psf_of(d, k) if psf is None else psf)
    s = _run(job, k, n)
    job.close()
    return s


def fresh(k, n):
    """the state of a fresh job after upload(D_b) and a run of kind k with n outer iterations; computed once"""
    if (k.id, n) not in _fresh:
        _fresh[(k.id, n)] = _fresh_run(k, n)
    return _fresh[(k.id, n)]


def _b_iterations(ia, ib):
    return (ia + ib) % 3 + 1


def _collect(failures, fn, *args):
    try:
        fn(*args)
    except AssertionError as e:
        failures.append(str(e).splitlines()[0])


# ---- P0 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ru.KINDS, ids=_id)
def test_p0_a_fresh_job_is_deterministic(k):
    d = ru.data(k.shape)["b"]
    for n in (1, 2, 3):
        a, b = _fresh_run(k, n), _fresh_run(k, n)
        if k.switch("fft_maxg") == 2:       # (the route flags ics_describe does not report)
            assert _get("maxg_launches") == 5 * n - 1
        elif k.route[0] == ru.TILES and k.switch("fft_conv2") and ru.SHAPES[k.shape][2] <= 25:
            assert _get("maxg_launches") == 0 and _get("maxg_scanned") == -1
        _eq(a, b, "%s, %d iterations, two fresh jobs" % (k.id, n))
        assert tuple(a["iterations"][[0, 1, 3]]) == (n, 0, 5 * n)
        # (one slot of keys per update pass: none on the small-frame kernel; fuse = 1 folds the pass into the next convolution, all of them in a
        #  blind run and all but the last of an outer iteration in a non-blind one)
        passes = 0 if k.route[0] == ru.SMALL or (k.fuse and k.blind) else (n if k.fuse else 5 * n)
        assert a["keys"].shape == (passes, 6)
        assert (a["scalars"][9] != 0) == k.blind        # (dtpsf: only a blind run steps the PSF)
        assert np.abs(a["u"] - d["u"]).max() > 0 and (not k.blind or np.abs(a["psf"] - ru.psf_of(d, k)).max() > 0)
        _fresh.setdefault((k.id, n), a)


# ---- P1 -------------------------------------------------------------------------------------------------------------------------------------
def _second_life(A, nA, B, nB, failures, progress=None, after_a=None):
    d = ru.data(A.shape)
    job = _new_job(A.shape)
    _upload(job, d["a"], A)
    sa = _run(job, A, nA, progress=progress)
    if after_a:
        after_a(sa)
    _upload(job, d["b"], B)
    s = _run(job, B, nB)
    job.close()
    _collect(failures, _eq, s, fresh(B, nB), "%s x %d, then %s x %d" % (A.id, sa["iterations"][0], B.id, nB))


@pytest.mark.parametrize("A", ru.KINDS, ids=_id)
def test_p1_second_life_behind_every_kind(A):
    ks = ru.kinds(A.shape)
    ia = ks.index(A)
    if A.shape == "S1":
        seq = [(B, ru.a_iterations("S1", ia, ib), _b_iterations(ia, ib)) for ib, B in enumerate(ks)]
        seq += [(ru.BY_ID[b], n, 2) for b in ru.FIXED_B for n in (1, 2, 3)]
    else:                  # (few kinds: every pair with every count)
        seq = [(B, n, _b_iterations(ia, ib)) for ib, B in enumerate(ks) for n in (1, 2, 3)]
    failures = []
    for B, nA, nB in seq:
        _second_life(A, nA, B, nB, failures)
    assert not failures, "%d of %d:\n%s" % (len(failures), len(seq), "\n".join(failures))


@pytest.mark.parametrize("cond", ["undo", "correlation"])
@pytest.mark.parametrize("A", [ru.BY_ID[i] for i in ru.SPECIAL_A], ids=_id)
def test_p1_second_life_behind_an_undone_and_a_frozen_run(A, cond):
    """undo: the callback ends run A at outer iteration 1 of 3 while iteration 2 is queued on the overlapped loop and is dropped (u / ut and e / e2
    exchanged back, the PSF restored from psf_bak, the tables repacked).  correlation = 1: run A leaves the caller's PSF detached (flags[0])."""
    ks = ru.kinds("S1")
    failures = []
    for ib, B in enumerate(ks):
        if cond == "undo":
            def ended(sa):
                assert tuple(sa["iterations"][[0, 1, 3]]) == (1, 2, 5), sa["iterations"]
            _second_life(A.with_(overlap=2), 3, B, _b_iterations(1, ib), failures, progress=lambda it, *rest: it == 1, after_a=ended)
        else:
            _second_life(A.with_(correlation=1), ib % 3 + 1, B, _b_iterations(2, ib), failures)
    assert not failures, "%d of %d:\n%s" % (len(failures), len(ks), "\n".join(failures))


# ---- P2 -------------------------------------------------------------------------------------------------------------------------------------
def _mixed_rows(shape):
    d = ru.data(shape)
    r0, nr = ru.ROWS
    image = d["a"]["image"].copy()
    image[r0:r0 + nr] = d["b"]["image"][r0:r0 + nr]
    return image


def _device_frames(shape, k):
    """D_b's image and u inside larger device images, at non-zero origins"""
    from lib import _native as nv
    d = ru.data(shape)["b"]
    rng = np.random.default_rng(5)
    big_f = rng.random((d["image"].shape[0] + 9, d["image"].shape[1] + 12, 3), dtype=np.float32)
    big_u = rng.random((d["u"].shape[0] + 5, d["u"].shape[1] + 8, 3), dtype=np.float32)
    fo, uo = (4, 7), (2, 3)
    big_f[fo[0]:fo[0] + d["image"].shape[0], fo[1]:fo[1] + d["image"].shape[1]] = d["image"]
    big_u[uo[0]:uo[0] + d["u"].shape[0], uo[1]:uo[1] + d["u"].shape[1]] = d["u"]
    return nv.DeviceImage.from_host(big_f), fo, nv.DeviceImage.from_host(big_u), uo, big_u


CHANNELS = ("write", "write_rows", "copy_rows", "upload_img", "tv_mode_1")


@pytest.mark.parametrize("channel", CHANNELS)
@pytest.mark.parametrize("k", [ru.BY_ID[i] for i in ru.IMAGE_COPY], ids=_id)
def test_p2_every_way_to_change_the_image(k, channel):
    from lib import _native as nv
    d = ru.data(k.shape)
    r0, nr = ru.ROWS
    job = _new_job(k.shape)
    _upload(job, d["a"], k)
    _run(job, k, 2)
    if channel == "write":
        job.write(nv.BUF_IMAGE, d["b"]["image"])
        image = d["b"]["image"]
    elif channel == "write_rows":
        job.write_rows(nv.BUF_IMAGE, r0, d["b"]["image"][r0:r0 + nr])
        image = _mixed_rows(k.shape)
    elif channel == "copy_rows":
        other = _new_job(k.shape)
        _upload(other, d["b"], k)
        job.copy_rows_from(nv.BUF_IMAGE, r0, other, nv.BUF_IMAGE, r0, nr)
        other.close()
        image = _mixed_rows(k.shape)
    elif channel == "upload_img":
        f_dev, fo, u_dev, uo, _ = _device_frames(k.shape, k)
        job.upload_img(f_dev, fo, u_dev, uo, ru.psf_of(d["b"], k))
        f_dev.close(); u_dev.close()
        image = d["b"]["image"]
    else:
        _run(job, ru.BY_ID[ru.IMAGE_STEPPER[k.shape]], 1)
        image = job.read(nv.BUF_IMAGE)
        print("tv_mode 1 moved %.1f %% of the image" % (100 * np.mean(image != d["a"]["image"])))
        assert np.any(image != d["a"]["image"])                 # (the run has stepped the image)
    assert np.array_equal(job.read(nv.BUF_IMAGE), image)
    job.write(nv.BUF_U, d["b"]["u"])
    job.write(nv.BUF_PSF, ru.psf_of(d["b"], k))
    s = _run(job, k, 2)
    job.close()
    _eq(s, _fresh_run(k, 2, image=image), "%s, image changed through %s" % (k.id, channel))


def test_p2_download_img_writes_the_window_and_nothing_else():
    k = ru.BY_ID["ti-bl"]
    job = _new_job(k.shape)
    _upload(job, ru.data(k.shape)["b"], k)
    _run(job, k, 2)
    f_dev, _, u_dev, uo, big_u = _device_frames(k.shape, k)
    job.download_img(u_dev, uo)
    got = u_dev.to_host()
    u = job.download()[0]
    job.close(); f_dev.close(); u_dev.close()
    assert np.array_equal(u.view(np.uint32), fresh(k, 2)["u"].view(np.uint32))
    inside = np.zeros(big_u.shape[:2], bool)
    inside[uo[0]:uo[0] + u.shape[0], uo[1]:uo[1] + u.shape[1]] = True
    assert np.array_equal(got[inside].view(np.uint32), u.reshape(-1, 3).view(np.uint32))
    assert np.array_equal(got[~inside].view(np.uint32), big_u[~inside].view(np.uint32))


@pytest.mark.parametrize("conv", [0, 2, 3], ids=["auto", "matrix", "tiles"])
def test_p2_device_call_behind_a_host_call_on_the_cached_job(conv):
    """lib.deconvolution keeps jobs by shape: richardson_lucy_MM with D_a, then richardson_lucy_MM_device with D_b on the same job, equals the
    device call alone"""
    from lib import deconvolution as dc
    M, N, MK = ru.SHAPES["S1"]
    d = ru.data("S1")
    win = ru.window("S1")

    def device_call():
        f_dev, fo, u_dev, uo, _ = _device_frames("S1", None)
        psf = d["b"]["psf_blind"].copy()
        with contextlib.redirect_stdout(io.StringIO()):
            dc.richardson_lucy_MM_device(f_dev, fo, u_dev, uo, psf, *win, 1e9, M, N, 3, MK, 2, ru.STEP, 10000.0, blind=True, conv=conv)
        out = u_dev.to_host()
        f_dev.close(); u_dev.close()
        return out, psf

    dc._drop_jobs()
    u_a, psf_a = d["a"]["u"].copy(), d["a"]["psf_blind"].copy()
    with contextlib.redirect_stdout(io.StringIO()):
        dc.richardson_lucy_MM(d["a"]["image"].copy(), u_a, psf_a, *win, 1e9, M, N, 3, MK, 3, ru.STEP, 10000.0, blind=True, conv=conv)      # (the same route: its copies of the image are D_a's)
    assert len(dc._job_cache) == 1
    used = device_call()
    assert len(dc._job_cache) == 1
    dc._drop_jobs()
    alone = device_call()
    dc._drop_jobs()
    assert np.array_equal(used[0].view(np.uint32), alone[0].view(np.uint32)) and np.array_equal(used[1].view(np.uint32), alone[1].view(np.uint32))
    assert np.abs(used[1] - d["b"]["psf_blind"]).max() > 0


# ---- P3 -------------------------------------------------------------------------------------------------------------------------------------
def _stages(job, conv):
    """one teacher-forced inner iteration, stage by stage -> {name: array} of what each stage writes, and every buffer at the end"""
    from lib import _native as nv
    p = job.params(*ru.window("S1"), 1e9, 1, ru.STEP, 10000.0, blind=True, conv=conv, stop_test=2)
    out = {}
    plan = ((nv.STAGE_SYNTH_RESIDUAL, "synth", ((nv.BUF_ERROR, slice(None)),)),
            (nv.STAGE_BACKPROJECT, "backproject", ((nv.BUF_GRADU, slice(None)), (nv.BUF_RED, slice(0, 6)))),
            (nv.STAGE_UPDATE, "update", ((nv.BUF_U, slice(None)), (nv.BUF_SCALARS, slice(0, 9)), (nv.BUF_RED, slice(12, 15)))),
            (nv.STAGE_PSF_GRADIENT, "gradk", ((nv.BUF_GRADK, slice(None)),)),
            (nv.STAGE_PSF_UPDATE, "psf", ((nv.BUF_PSF, slice(None)), (nv.BUF_SCALARS, slice(9, 10)))),
            (nv.STAGE_STATS, "stats", ((nv.BUF_SCALARS, slice(10, 15)),)))
    for stage, name, reads in plan:
        job.stage(stage, p)
        for buf, sl in reads:
            out["%s/%d" % (name, buf)] = job.read(buf)[sl].copy()
    for buf in (nv.BUF_ERROR, nv.BUF_GRADU, nv.BUF_U, nv.BUF_GRADK, nv.BUF_PSF, nv.BUF_SCALARS, nv.BUF_RED):
        out["end/%d" % buf] = job.read(buf)
    out["end/psf_caller"] = job.download()[2]
    return out


def _stage_inputs():
    d = ru.data("S1")["b"]
    ut = (d["u"] * np.float32(0.9) + np.float32(0.01)).astype(np.float32)
    return d, ut


def _set_frames(job, path):
    from lib import _native as nv
    d, ut = _stage_inputs()
    if path == "upload":
        job.upload(d["image"], d["u"], d["psf_blind"])
    else:
        job.write(nv.BUF_IMAGE, d["image"]); job.write(nv.BUF_U, d["u"]); job.write(nv.BUF_PSF, d["psf_blind"])
    job.write(nv.BUF_UT, ut)


_fresh_stages = {}


@pytest.mark.parametrize("path", ["upload", "write"])
@pytest.mark.parametrize("conv", [1, 2, 3], ids=["vector", "matrix", "tiles"])
@pytest.mark.parametrize("A", ru.STAGE_A)
def test_p3_stages_on_a_used_job(A, conv, path):
    """ics_rl_write of a PSF repacks the tables but, unlike ics_rl_upload, leaves flags[0] (frozen: the caller's PSF is detached) and psf_caller
    alone.  A frozen flag left by a run with correlation = 1 does reach ICS_STAGE_PSF_UPDATE: every buffer ics_rl_read returns is the fresh job's,
    and the caller's PSF of ics_rl_download stays what the run left -- the flag means nothing else (include/ics_hip.h, ics_rl_write)."""
    k = ru.BY_ID[A]
    frozen = A == "mx-fused"
    if frozen:
        k = k.with_(correlation=1)
    if (conv, path) not in _fresh_stages:
        job = _new_job("S1")
        _set_frames(job, path)
        _fresh_stages[(conv, path)] = _stages(job, conv)
        job.close()
    want = _fresh_stages[(conv, path)]
    job = _new_job("S1")
    _upload(job, ru.data("S1")["a"], k)
    _run(job, k, 2)
    caller_before = job.download()[2]
    _set_frames(job, path)
    got = _stages(job, conv)
    job.close()
    assert np.array_equal(want["end/psf_caller"], want["end/5"]) and np.abs(want["end/5"] - ru.data("S1")["b"]["psf_blind"]).max() > 0
    if frozen and path == "write":          # (the one difference, as documented)
        assert np.array_equal(got.pop("end/psf_caller"), caller_before) and not np.array_equal(caller_before, want["end/psf_caller"])
        want = {key: v for key, v in want.items() if key != "end/psf_caller"}
    _same(got, want, "stages behind %s, conv %d, frames by %s" % (k.id, conv, path))


# ---- P4 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [ru.BY_ID[i] for i in ru.READ_KINDS], ids=_id)
def test_p4_reads_after_a_run(k):
    """ICS_BUF_U = what ics_rl_download gives, ICS_BUF_IMAGE = the upload, ICS_BUF_PSF = the local PSF, ICS_BUF_GRADK = a fresh job's, on a fresh job
    and on a used one; ICS_BUF_UT = u as the last outer iteration found it (u of a run one iteration shorter) -- except behind a run on the
    transform tiles, where the frame behind it is not converted back from its mirror (include/ics_hip.h)."""
    from lib import _native as nv
    d = ru.data(k.shape)
    A = ru.kinds(k.shape)[0] if ru.kinds(k.shape)[0] is not k else ru.kinds(k.shape)[1]
    for n in (1, 2, 3):
        reads = []
        for used in (False, True):
            job = _new_job(k.shape)
            if used:
                _upload(job, d["a"], A)
                _run(job, A, n)
            _upload(job, d["b"], k)
            _run(job, k, n)
            u, psf, _ = job.download()
            r = {b: job.read(b) for b in (nv.BUF_U, nv.BUF_UT, nv.BUF_IMAGE, nv.BUF_PSF, nv.BUF_GRADK)}
            job.close()
            what = "%s x %d, %s job" % (k.id, n, "used" if used else "fresh")
            assert np.array_equal(r[nv.BUF_U].view(np.uint32), u.view(np.uint32)), what
            assert np.array_equal(u.view(np.uint32), fresh(k, n)["u"].view(np.uint32)), what
            assert np.array_equal(r[nv.BUF_IMAGE], d["b"]["image"]), what
            assert np.array_equal(r[nv.BUF_PSF].view(np.uint32), psf.view(np.uint32)), what
            before = d["b"]["u"] if n == 1 else fresh(k, n - 1)["u"]
            ut_is_previous_u = np.array_equal(r[nv.BUF_UT].view(np.uint32), before.view(np.uint32))
            if k.route[0] == ru.TILES:
                print("%s: ICS_BUF_UT %s u of the iteration before" % (what, "equals" if ut_is_previous_u else "is not"))
            else:
                assert ut_is_previous_u, what
            reads.append(r)
        assert np.array_equal(reads[0][nv.BUF_GRADK].view(np.uint32), reads[1][nv.BUF_GRADK].view(np.uint32)), "%s x %d: gradk" % (k.id, n)
        assert np.abs(reads[0][nv.BUF_GRADK]).max() > 0
