"""Mode 2 of the transform tiles (k_conv_fft<2>, A1 + A2 + A3 in one unit per tile pair): the far edge of its tile grid.

The last tile of an axis also stores the strip of the pad ring behind it -- up to 2 pad rows / columns -- wherever that saves the tile row /
column the strip would otherwise need (csrc/ics_conv_fft.hip: tile_rows, ics_conv_fft_fill_args).  Shapes (V = valid pixels per tile):

  a  100 x 100, 15   V 100: ext = 14 = 2 pad on both axes, ONE tile stores the 114^2 frame (the limit)
  b   96 x 196, 15   ext = 10 on both axes (one tile row, two tile columns) -- 4096^2 / 15 has this ext
  c  150 x  96, 15   columns extended, rows at the plain geometry (two tile rows either way)
  d  110 x 110,  9   V 112, 2 pad = 8, ext = 6
  e   75 x  75, 25   V 80, the widest PSF mode 2 serves in the loop, ext = 19 <= 24
  f  150 x 150, 15   no extension on either axis: the plain two-by-two grid, bit for bit what it gave before the extension existed
                     (tests/golden/fft_far_edge_f.npz, written by the commit before it)

Gates: those of tests/test_gpu_fft.py -- the one-unit stage against float64 sums formed from u and the image alone
(test_synthesis_and_back_projection_in_one_unit), whole runs with the unit switched on and off
(test_whole_run_with_one_unit_per_tile_pair_equals_the_two_kernel_run)."""
import contextlib
import io
import os

import numpy as np
import pytest

import rl_mm_oracle as orc
from helpers import conv_valid64, corr_full64, rel_err

CONV_TOL = 5e-6
FFT = 3

#        M,   N,  K, (ext_y, ext_x), units
CASES = {"a": (100, 100, 15, (14, 14), 3),
         "b": (96, 196, 15, (10, 10), 3),
         "c": (150, 96, 15, (0, 10), 3),
         "d": (110, 110, 9, (6, 6), 3),
         "e": (75, 75, 25, (19, 19), 3),
         "f": (150, 150, 15, (0, 0), 6)}


def grid(M, N, K):
    """tile rows, tile columns, ext_y, ext_x as the issue derives them: ceil(M / V) tiles where the rest of the u-frame is at most 2 pad"""
    pad, vy = K // 2, 128 - 2 * K + 2
    vx = vy & ~3
    out = []
    for m, v in ((M, vy), (N, vx)):
        full, short = -(-(m + 2 * pad) // v), -(-m // v)
        out.append((short, m + 2 * pad - short * v) if short < full else (full, 0))
    return out[0][0], out[1][0], out[0][1], out[1][1], vy, vx


@pytest.mark.parametrize("name", sorted(CASES))
def test_unit_count_of_the_cases(name):
    from lib import _native as nv
    M, N, K, ext, units = CASES[name]
    ty, tx, ey, ex, _, _ = grid(M, N, K)
    assert (ey, ex) == ext
    assert nv.conv2_units(M, N, K) == units == 3 * ((ty * tx + 1) // 2)


def test_unit_count_of_the_headline_and_of_frames_without_extension():
    from lib import _native as nv
    assert nv.conv2_units(4096, 4096, 15) == 2523           # 41 x 41 tiles: ten rounds on 256 workgroups (42 x 42 = 2646 units: eleven)
    assert nv.conv2_units(520, 610, 15) == 63               # 534 x 624: six by seven tiles with or without the pad ring
    assert nv.conv2_units(700, 820, 15) == 96               # rows 8 -> 7 (ext 14), columns 9 either way
    assert nv.conv2_units(6144, 6144, 31) == 12423          # 91 x 91 tiles of 68: 6174 = 90 x 68 + 54, nothing to save
    assert nv.conv2_units(2048, 2048, 65) == 0              # no mode 2 at this size (no valid pixels left)


def make_job(M, N, MK, seed=0):
    from lib import _native
    case = orc.synth_case(M, N, MK, seed=seed, per_channel_psf=True)
    rng = np.random.default_rng(seed + 1)
    psf = (case["psf0"] * (0.5 + rng.random(case["psf0"].shape, dtype=np.float32))).astype(np.float32)   # no symmetry: flips show
    orc.normalize_kernel(psf, MK)
    job = _native.RLJob(M, N, MK)
    job.upload(case["image"], case["u0"], psf)
    return job, case, psf


def key_to_float(k):   # ics_key2f (csrc/ics_common.h)
    k = int(k)
    return np.array([(k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)], np.uint32).view(np.float32)[0]


def one_unit_stage(M, N, MK, seed, tv=None):
    """The stage on a fresh job: returns what the gates need.  u = u0 + noise, the majoriser = u0, gradu pre-filled with 3."""
    from lib import _native as nv
    job, case, psf = make_job(M, N, MK, seed=seed)
    rng = np.random.default_rng(7)
    u = (case["u0"] + 0.01 * rng.standard_normal(case["u0"].shape)).astype(np.float32)
    job.write(nv.BUF_U, u)
    job.write(nv.BUF_UT, case["u0"])
    p = job.params(1, 5, 1, 5, 1e9, 1, 1e-3, 10000.0, blind=False, conv=FFT)
    conv = conv_valid64(u, psf)
    g_ref = corr_full64(conv - case["image"].astype(np.float64), psf)
    job.stage(nv.STAGE_SYNTH_RESIDUAL, p)
    job.stage(nv.STAGE_BACKPROJECT, p)
    g2 = job.read(nv.BUF_GRADU)
    job.write(nv.BUF_GRADU, np.full_like(u, 3.0))           # a pixel no unit stores keeps the 3
    job.stage(nv.STAGE_SYNTH_BACKPROJECT, p)
    g, red = job.read(nv.BUF_GRADU), job.red_keys()[:6].copy()
    assert np.array_equal(job.read(nv.BUF_U), u)
    job.close()
    return dict(u=u, ut=case["u0"], g=g, g2=g2, g_ref=g_ref, red=red, conv_max=float(np.max(np.abs(conv))))


def assert_stage_gates(r, label):
    """test_synthesis_and_back_projection_in_one_unit's gates: relative to max |gradu| three times the two kernels' error (+ 1e-6), absolute
    the convolutions' stage gate, the six maxima exactly those of the stage's own output"""
    err, err2 = rel_err(r["g"], r["g_ref"]), rel_err(r["g2"], r["g_ref"])
    worst = float(np.max(np.abs(r["g"] - r["g_ref"])))
    print("%s: one unit %.2e, two kernels %.2e (of max |gradu| = %.2e), max |d| = %.2e of the gate %.2e" % (
        label, err, err2, np.max(np.abs(r["g_ref"])), worst, CONV_TOL * r["conv_max"]))
    assert err < 3 * err2 + 1e-6 and worst < CONV_TOL * r["conv_max"]
    gg = (np.float32(10000.0) * r["g"] + (r["u"] - r["ut"]) * np.float32(0.5)).astype(np.float32)
    for c in range(3):
        assert key_to_float(r["red"][c]) == np.max(np.abs(gg[..., c]))
        assert key_to_float(r["red"][3 + c]) == np.max(r["u"][..., c])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_extended_tiles_against_float64(name):
    """gradu and the six maxima of the one-unit stage on the extended grids, the strips behind the last tile's own V rows / columns on their own:
    a strip left unwritten (3.0) or written as zeros cannot hide under a frame-wide maximum"""
    M, N, MK, ext, _ = CASES[name]
    ty, tx, ey, ex, vy, vx = grid(M, N, MK)
    r = one_unit_stage(M, N, MK, seed=MK + M)
    assert_stage_gates(r, "%s %dx%d K=%d" % (name, M, N, MK))
    d = np.abs(r["g"] - r["g_ref"])
    gate = CONV_TOL * r["conv_max"]
    for axis, e, first in ((0, ey, ty * vy), (1, ex, tx * vx)):
        if not e:
            continue
        sl = (slice(first, None), slice(None)) if axis == 0 else (slice(None), slice(first, None))
        assert r["g"][sl].shape[axis] == e                       # the strip reaches the u-frame's last row / column
        ref_max, got = float(np.max(np.abs(r["g_ref"][sl]))), float(np.max(d[sl]))
        print("  strip behind %s %d (%d wide): max |d| = %.2e, max |gradu| there = %.2e" % ("row" if axis == 0 else "column", first, e, got, ref_max))
        assert ref_max > 100 * gate                                # the reference is far from zero there: zeros would not pass
        assert got < gate
        for i in range(e):                                         # ... and in every single row / column of it
            one = (slice(first + i, first + i + 1), slice(None)) if axis == 0 else (slice(None), slice(first + i, first + i + 1))
            assert float(np.max(d[one])) < gate and float(np.max(np.abs(r["g"][one]))) > 0


def exact_inputs(M, N, MK, seed):
    """u, majoriser, image and PSF as small integers over powers of two: the same bits on every machine, whatever numpy it has"""
    rng = np.random.default_rng(seed)
    pad = MK // 2
    u = (rng.integers(1 << 12, 1 << 16, (M + 2 * pad, N + 2 * pad, 3)) / np.float32(1 << 16)).astype(np.float32)
    ut = (u + rng.integers(-8, 9, u.shape) / np.float32(1 << 16)).astype(np.float32)
    image = (rng.integers(1 << 12, 1 << 16, (M, N, 3)) / np.float32(1 << 16)).astype(np.float32)
    psf = (rng.integers(1, 1 << 8, (MK, MK, 3)) / np.float32(MK * MK << 7)).astype(np.float32)
    return u, ut, image, psf


def exact_stage(M, N, MK, seed):
    from lib import _native as nv
    u, ut, image, psf = exact_inputs(M, N, MK, seed)
    job = nv.RLJob(M, N, MK)
    job.upload(image, u, psf)
    job.write(nv.BUF_UT, ut)
    p = job.params(1, 5, 1, 5, 1e9, 1, 1e-3, 10000.0, blind=False, conv=FFT)
    job.write(nv.BUF_GRADU, np.full_like(u, 3.0))
    job.stage(nv.STAGE_SYNTH_BACKPROJECT, p)
    g, red = job.read(nv.BUF_GRADU), np.asarray(job.red_keys()[:6]).astype(np.uint32)
    job.close()
    return g, red


@pytest.mark.gpu
def test_frame_without_extension_keeps_its_bits(golden_dir):
    """case f: no tile row or column to save -- the geometry, hence every bit of gradu and of the six maxima, is what it was before the
    far-edge extension (the fixture was written by the commit before it from the same integer-valued inputs); and the stage's usual gates"""
    M, N, MK, ext, units = CASES["f"]
    assert grid(M, N, MK)[:4] == (2, 2, 0, 0)
    r = one_unit_stage(M, N, MK, seed=MK + M)
    assert_stage_gates(r, "f %dx%d K=%d" % (M, N, MK))
    z = np.load(os.path.join(golden_dir, "fft_far_edge_f.npz"))
    g, red = exact_stage(M, N, MK, seed=int(z["seed"]))
    assert np.array_equal(g.view(np.uint32), z["gradu"].view(np.uint32))
    assert np.array_equal(red, z["red"])


@pytest.mark.gpu
def test_few_persistent_workgroups_walk_extended_units(debug_switch):
    """396 x 496, 15 x 15: four by five tiles with ext = 10 on both axes (five by six without), interior units (tiles (1,1)+(1,2), (2,1)+(2,2))
    between outer-ring and extended ones on the same workgroup: five workgroups, then two, for thirty units, against the full grid bit for bit"""
    from lib import _native as nv
    M, N, MK = 396, 496, 15
    assert grid(M, N, MK)[:4] == (4, 5, 10, 10) and nv.conv2_units(M, N, MK) == 30
    job, case, psf = make_job(M, N, MK, seed=9)
    rng = np.random.default_rng(5)
    u = (case["u0"] + 0.01 * rng.standard_normal(case["u0"].shape)).astype(np.float32)
    job.write(nv.BUF_U, u); job.write(nv.BUF_UT, case["u0"])
    p = job.params(1, 5, 1, 5, 1e9, 1, 1e-3, 10000.0, blind=True, conv=FFT)
    res = {}
    for wgs in (5, 2, 0):
        debug_switch("max_wgs", wgs)
        job.write(nv.BUF_GRADU, np.full_like(u, 3.0))
        job.stage(nv.STAGE_SYNTH_BACKPROJECT, p)
        res[wgs] = (job.read(nv.BUF_GRADU), job.red_keys()[:6].copy())
    for wgs in (5, 2):
        assert np.array_equal(res[wgs][0], res[0][0]) and np.array_equal(res[wgs][1], res[0][1])      # the walk does not change a bit
    conv = conv_valid64(u, psf)
    g_ref = corr_full64(conv - case["image"].astype(np.float64), psf)
    d = np.abs(res[5][0] - g_ref)
    gate = CONV_TOL * np.max(np.abs(conv))
    print("5 workgroups: max |d| = %.2e, behind row 400 %.2e, behind column 500 %.2e, gate %.2e" % (d.max(), d[400:].max(), d[:, 500:].max(), gate))
    assert d.max() < gate and d[400:].max() < gate and d[:, 500:].max() < gate
    assert np.max(np.abs(g_ref[400:])) > 100 * gate and np.max(np.abs(g_ref[:, 500:])) > 100 * gate
    job.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,tv_mode", [("a", 0), ("b", 0), ("c", 0), ("d", 0), ("e", 0), ("b", 2)])
def test_whole_blind_run_on_extended_tiles_equals_the_two_kernel_run(name, tv_mode, debug_switch):
    """ics_rl_run, blind, three outer iterations, with A1 + A3 as one unit per tile pair (fft_conv2 = 1: extended tiles) against the same run
    with the two kernels (fft_conv2 = 0: modes 0 and 1, no extension anywhere) -- u and PSF within 1e-5, the stop-test scalars within 2e-3;
    the PAM kind (tv_mode 2: k_conv_fft<2, true>, G = T + lambd gradu stored over the extended tiles) on case b"""
    from lib import deconvolution as dc
    M, N, MK, _, _ = CASES[name]
    case = orc.synth_case(M, N, MK, seed=MK, blind=True)
    res = {}
    for sw in (1, 0):
        debug_switch("fft_conv2", sw)
        dc._drop_jobs()
        u, psf, image = case["u0"].copy(), case["psf0"].copy(), case["image"].copy()
        with contextlib.redirect_stdout(io.StringIO()):
            dc.richardson_lucy_MM(image, u, psf, *orc.default_window(M, N, MK), 1e9, M, N, 3, MK, 3, 1e-3, 10000.0, blind=True, conv=FFT, tv_mode=tv_mode)
        st = dc.richardson_lucy_MM.last
        assert st.iterations_done == 3 and not st.has_nan
        res[sw] = (u, psf, np.array(st.trace_M_r[:3]), np.array(st.trace_Hu[:3]), np.array(st.trace_varu[:3]))
    eu, ep = rel_err(res[1][0], res[0][0]), rel_err(res[1][1], res[0][1])
    print("%s %dx%d K=%d tv_mode=%d: one unit vs two kernels u %.2e psf %.2e" % (name, M, N, MK, tv_mode, eu, ep))
    print("  M_r %s / %s  Hu %s / %s  varu %s / %s" % (res[1][2], res[0][2], res[1][3], res[0][3], res[1][4], res[0][4]))
    assert eu < 1e-5 and ep < 1e-5
    for k in (2, 3, 4):
        np.testing.assert_allclose(res[1][k], res[0][k], rtol=2e-3)
    dc._drop_jobs()
