"""Mode 2 of the transform tiles without the epilogue's operand reads (csrc/ics_maxg_select.h; switch fft_maxg / ICS_FFT_MAXG): behind an
update pass of the run the launch is k_conv_fft<3>, max u comes from that update pass (k_update_planar) and max |g| from k_maxg_select on
the tiles the skip rule cannot exclude.  The launch it replaces -- k_conv_fft<2> with u and ut under every output quad -- stays behind the
switch, and everything here is held against it BIT FOR BIT after two outer iterations (ten inner ones), blind and non-blind:

  * the six reduction keys of EVERY inner iteration (debug switch key_trace), the step sizes dt they give, u, the PSFs and the traces;
  * frames with interior, rim and extended far-edge tiles and a single tile row (230 x 260, 100 x 420 at 9 x 9 and 15 x 15), one 600 x 700;
  * the first launch of a run (it reads its operands: no update pass in front), the aliased first inner iteration of the second outer
    one (Dmax = 0), a run that ends through undo() with another run behind it;
  * a NaN in u, a NaN in the image, an inf in u; a black image (every tile qualifies: every |gradu| is exactly 0) and a grey one;
  * a frame whose max |g| sits in a tile that does not hold max |gradu|: a wide bump in u0 that the first update cancels (large u - ut, no
    gradient left) beside a narrow one that it does not -- the premise is checked stage by stage on the two-kernel path.

Scanned (tile, channel) pairs of the last launch on the smooth 600 x 700 frame, 15 x 15: 3 of 3 x 42 = 126 (test_scanned_pairs_on_a_smooth_frame).
"""
import ctypes as C

import numpy as np
import pytest

import rl_mm_oracle as orc

pytestmark = pytest.mark.gpu

STEP, LAMBD = 1e-3, 10000.0
_cases = {}


def _smooth(rng, M, N):
    """a smooth random picture in [0.1, 0.9]: 8 x 8 blocks, box-filtered"""
    small = rng.random((M // 8 + 3, N // 8 + 3, 3), dtype=np.float32)
    a = np.kron(small, np.ones((8, 8, 1), np.float32))
    for axis in (0, 1):
        for _ in range(2):
            a = (a + np.roll(a, 2, axis) + np.roll(a, -2, axis) + np.roll(a, 4, axis)) * np.float32(0.25)
    return np.ascontiguousarray(a[4:4 + M, 4:4 + N] * np.float32(0.8) + np.float32(0.1))


def _case(M, N, MK):
    """image, u0 (the image edge-padded), blind start PSF, true PSF; computed once per shape and never written to"""
    key = (M, N, MK)
    if key not in _cases:
        rng = np.random.default_rng(M + 7 * N + 31 * MK)
        image = _smooth(rng, M, N) + np.float32(1e-3) * rng.standard_normal((M, N, 3), dtype=np.float32)
        pad = MK // 2
        u0 = np.ascontiguousarray(np.pad(image, ((pad, pad), (pad, pad), (0, 0)), mode="edge"))
        out = (image, u0, orc.uniform_psf(MK), orc.gaussian_psf(MK))
        for a in out:
            a.setflags(write=False)
        _cases[key] = out
    return _cases[key]


def _get(name):
    from lib import _native as nv
    v = C.c_int(0)
    assert nv.load().ics_debug_get(name.encode(), C.byref(v)) == 0, name
    return v.value


def _key_trace(job):
    from lib import _native as nv
    fn = nv.load().ics_debug_key_trace
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    fn.restype = C.c_int
    buf = np.zeros((64, 16), np.uint32)
    n = fn(job._h, buf.ctypes.data, 64)
    assert n >= 0
    return buf[:n, :6].copy()


def _state(job, st):
    from lib import _native as nv
    u, psf, caller = job.download()
    out = {"u": u, "psf": psf, "psf_caller": caller, "scalars": job.read(nv.BUF_SCALARS), "keys": _key_trace(job)}
    for name in st.TRACES:
        out["trace_" + name] = getattr(st, "trace_" + name)[:st.trace_len].copy()
    out["iterations"] = np.array([st.iterations_done, st.stopped, st.has_nan, st.inner_iterations], np.int32)
    return out


def _same(a, b, what, any_nan_in_statistics=False):
    """every bit of everything.  any_nan_in_statistics (frames that hold a NaN): where the window statistics are NaN in both runs, which NaN
    is not compared -- they are sums that atomics accumulate, and the sign of a NaN sum follows the order of its terms, in two runs of one
    build as well"""
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape, "%s: %s has shapes %s / %s" % (what, k, x.shape, y.shape)
        xb, yb = x.view(np.uint32), y.view(np.uint32)
        if any_nan_in_statistics and (k == "scalars" or k.startswith("trace_")):
            both = np.isnan(x) & np.isnan(y)
            xb, yb = np.where(both, 0, xb), np.where(both, 0, yb)
        assert np.array_equal(xb, yb), "%s: %s differs" % (what, k)


def _run(frames, MK, blind, maxg, debug_switch, iterations=2, step=STEP, lambd=LAMBD, progress=None, again=0):
    """one job, `iterations` outer iterations on the tiles (and `again` more in a second run), switch fft_maxg = maxg -> (states, counts)"""
    from lib import _native as nv
    debug_switch("fft_maxg", 2 if maxg else 0)      # (2: on frames of any size; the default, 1, starts at 6 Mpx)
    debug_switch("key_trace", 1)
    image, u0, psf = frames
    M, N = image.shape[:2]
    job = nv.RLJob(M, N, MK)
    job.upload(image, u0, psf)
    win = orc.default_window(M, N, MK)
    states = []
    for n in (iterations, again):
        if n:
            st = job.run(job.params(*win, 1e9, n, step, lambd, blind=blind, conv=nv.CONV_FFT, stop_test=2), progress=progress)
            states.append(_state(job, st))
            progress = None
    counts = {k: _get("maxg_" + k) for k in ("scanned", "pairs", "total", "launches")}
    job.close()
    return states, counts


def _on_off(frames, MK, blind, debug_switch, what, any_nan_in_statistics=False, **kw):
    on, counts = _run(frames, MK, blind, 1, debug_switch, **kw)
    off, _ = _run(frames, MK, blind, 0, debug_switch, **kw)
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        _same(a, b, "%s, run %d" % (what, i), any_nan_in_statistics)
    return on, counts


def _frames(M, N, MK, blind):
    image, u0, psf_uniform, psf_true = _case(M, N, MK)
    return image, u0, psf_uniform if blind else psf_true


SHAPES = [(230, 260, 9), (230, 260, 15), (100, 420, 9), (100, 420, 15), (600, 700, 15)]


@pytest.mark.parametrize("blind", [False, True], ids=["nonblind", "blind"])
@pytest.mark.parametrize("M,N,MK", SHAPES)
def test_two_outer_iterations_switch_on_and_off(M, N, MK, blind, debug_switch):
    """ten inner iterations: the first launch of the run reads its operands, the other nine do not -- the sixth is the aliased one"""
    on, counts = _on_off(_frames(M, N, MK, blind), MK, blind, debug_switch, "%dx%d/%d" % (M, N, MK))
    st = on[0]
    assert st["iterations"][0] == 2 and st["iterations"][3] == 10 and not st["iterations"][2]
    assert st["keys"].shape == (10, 6) and np.all(st["keys"] != 0)
    assert counts["launches"] == 9 and 0 < counts["total"] <= 9 * counts["pairs"]
    assert np.abs(st["u"] - _case(M, N, MK)[1]).max() > 0


def test_default_switch_leaves_small_frames_on_the_operand_reading_launch(debug_switch):
    from lib import _native as nv
    image, u0, psf = _frames(230, 260, 15, False)
    job = nv.RLJob(230, 260, 15)
    job.upload(image, u0, psf)
    debug_switch("fft_maxg", 1)
    job.run(job.params(*orc.default_window(230, 260, 15), 1e9, 1, STEP, LAMBD, blind=False, conv=nv.CONV_FFT))
    job.close()
    assert _get("maxg_launches") == 0 and _get("maxg_scanned") == -1


def test_scanned_pairs_on_a_smooth_frame(debug_switch):
    """600 x 700, 15 x 15, non-blind: 42 tiles x 3 channels = 126 pairs per launch.  Measured on an MI355X: 3 of 126 in the last launch and 27 over
    the run's nine operand-free launches -- one tile per channel, the one that holds max |gradu| (the count is printed here; NOTES_r08.md)."""
    M, N, MK = 600, 700, 15
    _, counts = _run(_frames(M, N, MK, False), MK, False, 1, debug_switch)
    print("scanned pairs, last launch: %d of %d; all %d launches: %d" % (counts["scanned"], counts["pairs"], counts["launches"], counts["total"]))
    assert counts["pairs"] == 126
    assert 0 < counts["scanned"] < counts["pairs"]


@pytest.mark.parametrize("blind", [False, True], ids=["nonblind", "blind"])
def test_undo_of_the_overlapped_loop_and_the_run_behind_it(blind, debug_switch):
    """the callback stops the run at outer iteration 2 while iteration 3 is queued and is undone; the next run starts with an
    operand-reading launch like every run"""
    M, N, MK = 230, 260, 15
    on, counts = _on_off(_frames(M, N, MK, blind), MK, blind, debug_switch, "undo", iterations=4, progress=lambda it, *rest: it == 2, again=1)
    assert on[0]["iterations"][0] == 2 and on[0]["iterations"][1] == 2
    assert on[1]["iterations"][0] == 1 and on[1]["keys"].shape == (5, 6)
    assert counts["launches"] == 4        # (the second run: five launches, the first of them with operands)


def _poisoned(kind, M, N, MK, blind):
    image, u0, psf = _frames(M, N, MK, blind)
    image, u0 = image.copy(), u0.copy()
    if kind == "nan_u":
        u0[120, 57, 1] = np.nan
    elif kind == "nan_image":
        image[31, 140, 2] = np.nan
    elif kind == "inf_u":
        u0[205, 199, 0] = np.inf
    return image, u0, psf


@pytest.mark.parametrize("blind", [False, True], ids=["nonblind", "blind"])
@pytest.mark.parametrize("kind", ["nan_u", "nan_image", "inf_u"])
def test_nan_and_inf_propagate_as_before(kind, blind, debug_switch):
    M, N, MK = 230, 260, 15
    on, counts = _on_off(_poisoned(kind, M, N, MK, blind), MK, blind, debug_switch, kind, any_nan_in_statistics=True)
    assert on[0]["iterations"][2] == 1                      # has_nan
    assert counts["launches"] == 9


@pytest.mark.parametrize("blind", [False, True], ids=["nonblind", "blind"])
@pytest.mark.parametrize("level", [0.0, 0.5], ids=["black", "grey"])
def test_constant_image(level, blind, debug_switch):
    """black: every convolution of zeros is exactly 0, so every tile has Gt = Gmax = 0 and Dmax = 0 -- hi' > 0 = lo, every tile is scanned in
    every launch.  grey: the residual is the rounding noise of the transforms, the same in every interior tile; how many tiles qualify is
    up to that noise (printed), the results are not."""
    M, N, MK = 230, 260, 15
    image = np.full((M, N, 3), level, np.float32)
    u0 = np.full((M + MK - 1, N + MK - 1, 3), level, np.float32)
    psf = orc.uniform_psf(MK) if blind else orc.gaussian_psf(MK)
    on, counts = _on_off((image, u0, psf), MK, blind, debug_switch, "constant %g" % level)
    print("constant %g: scanned pairs, last launch %d of %d; all %d launches: %d" % (level, counts["scanned"], counts["pairs"], counts["launches"], counts["total"]))
    assert counts["launches"] == 9 and counts["pairs"] == 27
    if level == 0.0:
        assert counts["scanned"] == counts["pairs"] and counts["total"] == 9 * counts["pairs"]
    else:
        assert 0 < counts["scanned"] <= counts["pairs"]


def _bumps(M, N, MK):
    """u0 = the image edge-padded + a wide bump (sigma 14 px, 0.3 high, centre of tile (0, 0) of the 100-pixel grid) + a narrow one (sigma 2.5 px --
    the PSF's --, 0.6 high, tile (1, 1)); lambd = 1 and step = 0.3 / max u0.  The PSF passes the wide bump whole and a third of the narrow one, so
    the first |g| peaks under the wide bump and the first update moves u there by step * max u = 0.3: the wide bump is gone (u - ut = -0.3, no
    gradient left), about half of the narrow one stays (gradient 0.1, u - ut = -0.3 as well but of the other sign than lambd * gradu)"""
    image, u0, _, psf = _case(M, N, MK)
    pad = MK // 2
    y, x = np.mgrid[0:M + 2 * pad, 0:N + 2 * pad].astype(np.float32)
    wide = np.exp(-((y - 50 - pad) ** 2 + (x - 50 - pad) ** 2) / (2 * 14.0 ** 2))
    narrow = np.exp(-((y - 150 - pad) ** 2 + (x - 150 - pad) ** 2) / (2 * 2.5 ** 2))
    u0 = (u0 + (np.float32(0.3) * wide + np.float32(0.6) * narrow)[..., None].astype(np.float32)).astype(np.float32)
    return (image, u0, psf), float(0.3 / u0.max()), 1.0


def test_maximum_of_g_in_a_tile_that_does_not_hold_gmax(debug_switch):
    from lib import _native as nv
    M, N, MK = 230, 260, 15
    frames, step, lambd = _bumps(M, N, MK)
    # the premise, on the two-kernel path stage by stage: after one update, |gradu| peaks under the narrow bump and |g| under the wide one
    job = nv.RLJob(M, N, MK)
    job.upload(*frames)
    p = job.params(*orc.default_window(M, N, MK), 1e9, 1, step, lambd, blind=False, conv=nv.CONV_FFT)
    job.stage(nv.STAGE_MAJORIZE, p)
    for stage in (nv.STAGE_SYNTH_RESIDUAL, nv.STAGE_BACKPROJECT, nv.STAGE_UPDATE, nv.STAGE_SYNTH_RESIDUAL, nv.STAGE_BACKPROJECT):
        job.stage(stage, p)
    gradu, u, ut = job.read(nv.BUF_GRADU), job.read(nv.BUF_U), job.read(nv.BUF_UT)
    job.close()
    g = np.float32(lambd) * gradu + (u - ut) * np.float32(0.5)
    tile = lambda a: tuple(int(v) // 100 for v in np.unravel_index(np.argmax(np.abs(a[..., 0])), a.shape[:2]))      # (V = Vy = 128 - 2 * 15 + 2)
    print("max |g| %.4f in tile %s, max |gradu| %.4f in tile %s" % (np.abs(g[..., 0]).max(), tile(g), np.abs(gradu[..., 0]).max(), tile(gradu)))
    assert tile(g) == (0, 0) and tile(gradu) == (1, 1), (tile(g), tile(gradu))
    on, counts = _on_off(frames, MK, False, debug_switch, "bumps", step=step, lambd=lambd)
    assert counts["launches"] == 9
