"""GPU: DeviceImage.align / align_sums / warp and lib.utils.align / warp / estimate_psf(register=) (csrc/ics_img_align.hip) against the
float64 specification (tests/align_ref.py).

align_sums (ar.SUMS_CASES: 31 x 33, one partial tile each way; 64 x 96; 97 x 121; a window inside it; a moving frame of another shape),
every model with and without the photometric terms, at a matrix that is no identity, gain 1.1 and bias -0.03:
|S - S_ref|_ij <= 1e-4 sqrt(S_ii S_jj), |g - g_ref|_i <= 1e-4 sqrt(S_ii sum r^2), sum r^2 within 1e-4 relative, the count exact.
warp (ar.WARP_CASES: 5 x 7, 33 x 65, 40 x 52 to 61 x 47, a line of 2040 px either way): the identity and an integer shift bit for bit, an
affine and a homography within the project's parity gate, 1e-4 max(1, max |ref|).
align on the recovery pairs of tests/test_align.py: the device's final matrix moves no corner more than 0.05 px from the
specification's -- a twentieth of the pixel estimate_psf needs; the float32 restatement of the whole loop, which tests/test_align.py
holds to a quarter of that, lies 2e-6 ... 8e-6 px from it, and so does the device -- and the steps per level are the specification's or one off.
tests/test_align.py shows the float32 evaluation of the specification within a quarter of each of these gates."""
import gc

import numpy as np
import pytest

import align_ref as ar

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def on_device(*arrays):
    from lib import _native
    return [_native.DeviceImage.from_host(a) for a in arrays]


def close(*images):
    for m in images:
        m.close()


@pytest.mark.parametrize("photometric", (True, False))
@pytest.mark.parametrize("model", list(ar.MODELS))
@pytest.mark.parametrize("case", range(len(ar.SUMS_CASES)))
def test_align_sums_match_the_float64_specification(case, model, photometric):
    shape_f, shape_m, window = ar.SUMS_CASES[case]
    moving, fixed = ar.sums_pair(shape_f, shape_m)
    M = ar.sums_matrix(shape_f, shape_m, window)
    S, g, rr, n = ar.sums_on_window(moving, fixed, M, window, model, photometric, ar.SUMS_GAIN, ar.SUMS_BIAS)
    dm, df = on_device(moving, fixed)
    try:
        Sd, gd, rrd, nd = dm.align_sums(df, M, model, photometric, ar.SUMS_GAIN, ar.SUMS_BIAS, window)
    finally:
        close(dm, df)
    d = np.sqrt(np.diag(S))
    eS, eg, er = (np.abs(Sd - S) / np.outer(d, d)).max(), (np.abs(gd - g) / (d * np.sqrt(rr))).max(), abs(rrd / rr - 1)
    print("align_sums %s against %s, window %s, %s, photometric %s: S %.3g, g %.3g, r^2 %.3g (gate %.3g); count %d" % (
        shape_f, shape_m, window, model, photometric, eS, eg, er, ar.GATE, nd))
    assert Sd.shape == S.shape and np.array_equal(Sd, Sd.T)
    assert nd == n
    assert eS <= ar.GATE and eg <= ar.GATE and er <= ar.GATE


@pytest.mark.parametrize("case", range(len(ar.SUMS_TRIP_CASES)))
def test_align_sums_where_the_reduction_runs_both_loop_forms(case):
    """ar.SUMS_TRIP_CASES: per variant a frame whose tiles number between 8 and 9 times the reduction's parts, so that every lane makes
    one eight-wide trip and some a tail step too, and the widest variant on 1190 tiles (ten trips, or nine and a tail of seven); the assertions
    and the gate of the test above"""
    shape, model, photometric = ar.SUMS_TRIP_CASES[case]
    moving, fixed, M, (S, g, rr, n) = ar.sums_trip_reference(case)
    dm, df = on_device(moving, fixed)
    try:
        Sd, gd, rrd, nd = dm.align_sums(df, M, model, photometric, ar.SUMS_GAIN, ar.SUMS_BIAS, None)
    finally:
        close(dm, df)
    d = np.sqrt(np.diag(S))
    eS, eg, er = (np.abs(Sd - S) / np.outer(d, d)).max(), (np.abs(gd - g) / (d * np.sqrt(rr))).max(), abs(rrd / rr - 1)
    print("align_sums %s, %d tiles, %s, photometric %s: S %.3g, g %.3g, r^2 %.3g (gate %.3g); count %d" % (
        shape, -(-shape[0] // ar.TILE) * -(-shape[1] // ar.TILE), model, photometric, eS, eg, er, ar.GATE, nd))
    assert Sd.shape == S.shape and np.array_equal(Sd, Sd.T)
    assert nd == n
    assert eS <= ar.GATE and eg <= ar.GATE and er <= ar.GATE


@pytest.mark.parametrize("shape_s,shape_o", ar.WARP_CASES)
def test_warp_matches_the_float64_specification(shape_s, shape_o):
    from lib import utils
    src = ar.warp_source(shape_s)
    (ds,) = on_device(src)
    try:
        same = ds.warp(np.eye(3))
        moved = ds.warp(ar.translation(2, -1))                         # out[y][x] = src[y - 1][x + 2]
        got_same, got_moved = same.to_host(), moved.to_host()
        close(same, moved)
        assert np.array_equal(bits(got_same), bits(src))
        assert np.array_equal(bits(got_moved[1:, :-2]), bits(src[:-1, 2:]))
        assert np.array_equal(bits(got_moved), bits(ar.warp(src, ar.translation(2, -1), dtype=np.float32)))   # the repeated edge too
        for name, M in ar.warp_matrices(shape_s, shape_o).items():
            ref = ar.warp(src, M, shape_o)
            out = ds.warp(M, shape_o)
            got = out.to_host()
            out.close()
            err, bound = np.abs(got - ref).max(), ar.GATE * max(1.0, np.abs(ref).max())
            print("warp %s -> %s, %s: max |gpu - ref| %.3g (gate %.3g)" % (shape_s, shape_o, name, err, bound))
            assert got.shape == shape_o + (3,) and got.dtype == np.float32
            assert err <= bound
            assert np.array_equal(bits(utils.warp(src, M, shape_o)), bits(got))                               # an array gives an array, the same bits
    finally:
        close(ds)


@pytest.mark.parametrize("model,blur", ar.RECOVERY)
def test_align_matches_the_float64_specification(model, blur):
    from lib import utils
    moving, fixed, M = ar.pair(model, blur)
    ref, per = ar.recovered(model, blur)
    got = utils.align(moving, fixed, model, info=True)
    gap, err = ar.corner_error(got.matrix, ref.matrix, fixed.shape), ar.corner_error(got.matrix, M, fixed.shape)
    print("align %s, box %d: %.3g px from the specification (gate %.2f), %.4f px from the truth (bound %.2f); %d steps against %s; gain %.5f / %.5f, bias %.5f / %.5f" % (
        model, blur, gap, ar.ALIGN_GATE, err, ar.RECOVERY_BOUND[model, blur], got.steps, per, got.gain, ref.gain, got.bias, ref.bias))
    assert got.matrix.shape == (3, 3) and got.matrix.dtype == np.float64 and got.matrix[2, 2] == 1.0
    assert gap <= ar.ALIGN_GATE
    assert err <= ar.RECOVERY_BOUND[model, blur]
    assert abs(got.steps - sum(per)) <= len(per)
    assert got.levels == ref.levels == len(per) and 0 <= got.last_step < 1e-3
    assert abs(got.gain - ref.gain) <= 1e-3 and abs(got.bias - ref.bias) <= 1e-3
    assert abs(got.rms / ref.rms - 1) <= 1e-3 and abs(got.coverage - ref.coverage) <= 1e-3


def test_steps_per_level_are_the_specifications_or_one_off():
    """a level at a time (levels=1 on the halved frames, then on the full ones from that start) so that the steps of each level show"""
    from lib import utils
    for model, blur in (("affine", 0), ("homography", 9)):
        moving, fixed, _ = ar.pair(model, blur)
        half = lambda pic: np.ascontiguousarray(np.dstack([ar.half(np.asarray(pic[..., c], np.float32)) for c in range(3)]))
        coarse_ref = ar.align(half(moving), half(fixed), model, levels=1)
        coarse = utils.align(half(moving), half(fixed), model, levels=1, info=True)
        start = ar.UP @ coarse_ref.matrix @ np.linalg.inv(ar.UP)
        fine_ref = ar.align(moving, fixed, model, levels=1, init=start)
        fine = utils.align(moving, fixed, model, levels=1, init=start, info=True)
        print("%s, box %d: steps %d / %d coarse, %d / %d fine (device / specification)" % (model, blur, coarse.steps, coarse_ref.steps, fine.steps, fine_ref.steps))
        assert abs(coarse.steps - coarse_ref.steps) <= 1 and abs(fine.steps - fine_ref.steps) <= 1
        assert coarse.levels == coarse_ref.levels == 1 and fine.levels == fine_ref.levels == 1
        three = utils.align(moving, fixed, model, levels=3, info=True)
        assert three.levels == ar.align(moving, fixed, model, levels=3).levels == 3
        assert ar.corner_error(fine.matrix, fine_ref.matrix, fixed.shape) <= ar.ALIGN_GATE


def test_a_window_an_init_and_frames_of_two_shapes():
    from lib import utils
    moving, fixed, M = ar.pair("affine", 0)
    window = (9, 150, 14, 181)
    cut = np.ascontiguousarray(moving[3:, :170])                        # moving loses three rows and 22 columns: M shifts by (0, -3)
    init = ar.translation(0.5, -3.5) @ ar.about_centre(ar.PAIR_SHAPE, 3.0, 1.02)
    ref = ar.align(cut, fixed, "affine", init=init, window=window)
    got = utils.align(cut, fixed, "affine", init=init, window=window, info=True)
    gap, err = ar.corner_error(got.matrix, ref.matrix, fixed.shape), ar.corner_error(got.matrix, ar.translation(0, -3) @ M, fixed.shape)
    print("window %s, moving %s: %.3g px from the specification, %.4f px from the truth, coverage %.3f / %.3f" % (window, cut.shape[:2], gap, err, got.coverage, ref.coverage))
    assert gap <= ar.ALIGN_GATE and err <= 0.1 and abs(got.coverage - ref.coverage) <= 1e-3


def test_two_runs_give_identical_bits_and_the_sources_are_untouched():
    moving, fixed, M = ar.pair("homography", 9)
    dm, df = on_device(moving, fixed)
    try:
        a1, a2 = dm.align(df, "homography"), dm.align(df, "homography")
        s1, s2 = dm.align_sums(df, a1.matrix, "homography", True, a1.gain, a1.bias), dm.align_sums(df, a1.matrix, "homography", True, a1.gain, a1.bias)
        w1, w2 = dm.warp(a1.matrix, fixed.shape), dm.warp(a1.matrix, fixed.shape)
        h1, h2 = w1.to_host(), w2.to_host()
        close(w1, w2)
        hm, hf = dm.to_host(), df.to_host()
    finally:
        close(dm, df)
    assert np.array_equal(bits(a1.matrix), bits(a2.matrix)) and a1[1:] == a2[1:]
    assert np.array_equal(bits(s1[0]), bits(s2[0])) and np.array_equal(bits(s1[1]), bits(s2[1])) and s1[2:] == s2[2:]
    assert np.array_equal(bits(h1), bits(h2))
    assert np.array_equal(bits(hm), bits(moving)) and np.array_equal(bits(hf), bits(fixed))


def test_arrays_and_device_images_agree_bit_for_bit():
    from lib import utils
    moving, fixed, _ = ar.pair("affine", 9)
    from_arrays = utils.align(moving, fixed, "affine", info=True)
    dm, df = on_device(moving, fixed)
    try:
        from_images = utils.align(dm, df, "affine", info=True)
        with pytest.raises(ValueError, match="both"):
            utils.align(dm, fixed)
        with pytest.raises(ValueError, match="both"):
            utils.align(moving, df)
        warped = utils.warp(dm, from_images.matrix, fixed.shape)
        host = warped.to_host()
        warped.close()
    finally:
        close(dm, df)
    assert np.array_equal(bits(from_arrays.matrix), bits(from_images.matrix)) and from_arrays[1:] == from_images[1:]
    assert np.array_equal(bits(utils.align(moving, fixed, "affine")), bits(from_arrays.matrix))
    assert np.array_equal(bits(utils.warp(moving, from_arrays.matrix, fixed.shape)), bits(host))


def test_on_poisoned_red_zoned_pool_blocks(debug_switch):
    """pool check mode (csrc/ics_pool.h): every block the calls take is filled with 0xFF (NaN) and its red zone verified when it goes
    back -- a read of a plane entry or a slot nobody wrote would make the sums NaN, a store past the workspace's end would be counted"""
    from lib import _native
    from lib import deconvolution as dc
    from lib import utils
    moving, fixed, _ = ar.pair("homography", 0)
    window = (3, 158, 5, 190)                                            # 155 x 185: partial tiles both ways, odd sides at both levels

    def run():
        got = utils.align(moving, fixed, "homography", window=window, info=True)
        return got, utils.warp(moving, got.matrix, (61, 47))

    clean, picture = run()
    dc._drop_jobs(); gc.collect()
    _native.debug_set("pool_overruns", 0)
    debug_switch("pool_check", 0xFF)
    poisoned, picture_p = run()
    gc.collect()
    debug_switch("pool_check", -1)
    gc.collect()
    assert _native.debug_set("pool_overruns", 0) == 0
    assert np.array_equal(bits(poisoned.matrix), bits(clean.matrix)) and poisoned[1:] == clean[1:]
    assert np.array_equal(bits(picture_p), bits(picture))


def test_refusals_and_their_messages():
    from lib import _native, utils
    moving, fixed, _ = ar.pair("translation", 0)
    with pytest.raises(ValueError, match="frames do not overlap enough"):
        utils.align(moving, fixed, init=ar.translation(400, 0))
    with pytest.raises(ValueError, match="frames do not overlap enough"):
        utils.align(moving, fixed, init=ar.translation(0, 130))
    for photometric in (True, False):
        with pytest.raises(ValueError, match="no texture to align on"):
            utils.align(np.full(moving.shape, 0.4, np.float32), fixed, "affine", photometric)
    for which in (0, 1):
        frames = [moving.copy(), fixed.copy()]
        frames[which][80, 90, 1] = np.nan
        with pytest.raises(ValueError, match="not finite: despeckle first"):
            utils.align(frames[0], frames[1], "translation")
    # ... and by the native entry itself: a box outside the fixed frame, frames of two contexts cannot be made here
    import ctypes as C
    dm, df = on_device(moving, fixed)
    M, gb, stats = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_double * 2)(1, 0), (C.c_double * 5)()
    rc_box = _native.load().ics_img_align(dm._h, df._h, 0, 161, 0, 192, 1, 1, 0, 30, 1e-3, M, gb, stats)
    rc_level = _native.load().ics_img_align(dm._h, df._h, 0, 160, 0, 192, 1, 1, 5, 30, 1e-3, M, gb, stats)
    close(dm, df)
    assert rc_box == _native.ICS_EINVAL and rc_level == _native.ICS_EINVAL


def test_estimate_psf_registers_device_frames_and_prints_its_line(capsys):
    """the pair of tests/test_align.py: L1 to the true 9 px box 0.111 from the registered pair, 0.115 after align + warp in the
    specification, 0.600 from the misregistered pair as it is; the line reads `Register : affine, 0.00041 px last step, rms 0.0313, coverage 96 %`"""
    from lib import utils
    K = 9
    sharp, blurred, off, M = ar.psf_pair(K)
    k = np.ones((K, K, 3)) / K ** 2
    l1 = lambda est: max(np.abs(est[..., c].astype(np.float64) - k[..., c]).sum() for c in range(3))
    db, ds, do = on_device(blurred.astype(np.float32), sharp.astype(np.float32), off.astype(np.float32))
    try:
        registered = l1(utils.estimate_psf(db, ds, K))
        left = l1(utils.estimate_psf(db, do, K))
        capsys.readouterr()
        got = utils.estimate_psf(db, do, K, register="affine", info=True)
        line = capsys.readouterr().out
        kept = do.to_host()
    finally:
        close(db, ds, do)
    print(line, "L1 to the true box: registered %.4f, register='affine' %.4f (corners %.3f px off), as it is %.4f" % (
        registered, l1(got.psf), ar.corner_error(got.matrix, M, ar.PAIR_SHAPE), left))
    import re
    assert re.fullmatch(r"Register : affine, [0-9.e-]+ px last step, rms 0\.\d{4}, coverage \d+ %\n", line), line
    assert l1(got.psf) <= 2 * registered and left >= 4 * registered
    assert ar.corner_error(got.matrix, M, ar.PAIR_SHAPE) <= 0.2
    assert np.array_equal(bits(kept), bits(off.astype(np.float32)))
    from_arrays = utils.estimate_psf(blurred.astype(np.float32), off.astype(np.float32), K, register="affine", info=True)
    assert np.array_equal(bits(from_arrays.psf), bits(got.psf)) and np.array_equal(bits(from_arrays.matrix), bits(got.matrix))
    assert utils.estimate_psf(blurred.astype(np.float32), sharp.astype(np.float32), K, info=True).matrix is None
