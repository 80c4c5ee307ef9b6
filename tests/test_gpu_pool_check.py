"""GPU: every kernel route on poisoned, red-zoned pool blocks (csrc/ics_pool.h, the debug switches pool_check / pool_overruns /
pool_selftest; the bookkeeping itself: tests/test_pool_host.py).

The context's block pool recycles freed blocks without clearing them and rounds every request up, so a read of memory nobody wrote
and a store past the end of a buffer both go unseen: a fresh hipMalloc returns zero pages, a recycled block holds the last test's
finite values, a stale value times a zero weight is 0, and the slack behind a buffer belongs to nobody.  In check mode every block
is filled with a byte when it is handed out and the bytes behind the request are compared with it when it comes back.

Fill bytes: 0xFF (float32 NaN, all-ones as a counter: stale x 0), 0x7F (3.39e38, finite: maxima, which fmaxf would let a NaN slip
past), 0xFE (-1.69e38: minima).

Per case: every cached job is dropped and every image closed, so that every buffer of the case is allocated under the switch; the
case runs twice with the switch off, once per fill byte, and the blocks go back to the pool, where their red zones are verified;
pool_overruns must still be 0.
 (a) the poisoned runs equal the unpoisoned run bit for bit (uint32 views; whole runs: also the iteration count, the stop flag, the
     has-NaN flag, the traces and the printed lines).  The two unpoisoned runs show whether the route is reproducible at all; one that is
     not goes on NOT_REPRODUCIBLE below with its reason and gets gate (b) only.  No image filter is on that list.
 (b) the poisoned run against the family's reference by the family's own gate, imported from its test module: whole runs by
     check_case of tests/test_gpu_route_matrix.py; filters by their derived bounds or bit equalities where the family has those (blurs,
     USM, noise estimate, despeckle, the exact operators), else by 4 x F32_RESTATEMENT_ERROR.  Those constants were measured on the
     family's own pictures, sizes and parameter sets, so they are applied there and nowhere else.  Where the size of a test is none of the
     family's (65 x 97 for most; 5 x 7 for the bilateral filter), or a setting the issue asks for has no constant (9 iterations of the TV
     denoiser, 3 wavelet scales), the same run() -- so the same poisoned pool -- also runs a measured parameter set on the family's
     picture of its nearest measured size (nearest_measured), and that is compared with the family's reference; the settings without a
     constant get the bit equality of the routes that the family's documentation promises on top.
No tolerance is new here: every gate is imported from the family's module."""
import contextlib
import ctypes as C
import functools
import gc
import io

import numpy as np
import pytest

import route_cases as rc
import test_gpu_route_matrix as rm

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x7F, 0xFE)
SIZES = [(5, 7), (65, 97), (301, 287)]
# Whole-run ids (of the parametrised tests below) whose two UNPOISONED runs differ in some bit, with the reason: gate (b) only.
NOT_REPRODUCIBLE = {}


# ---- the scaffold -----------------------------------------------------------------------------------------------------------------------
def quiesce():
    """no cached job, no image: everything goes back to the pool (where check-mode blocks are verified)"""
    from lib import deconvolution as dc
    dc._drop_jobs()
    gc.collect()


def bits(x):
    if isinstance(x, np.ndarray) and x.dtype.kind == "f":
        return np.ascontiguousarray(x).view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
    return x


def same_bits(a, b):
    """two results (nested tuples / lists / dicts of arrays and plain values) are equal, floats compared by their bits"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    if isinstance(a, float):
        return same_bits(np.array([a]), np.array([b]))
    return a == b


def first_difference(a, b, path=""):
    if isinstance(a, dict):
        for k in a:
            if not same_bits(a[k], b.get(k)):
                return first_difference(a[k], b[k], "%s[%r]" % (path, k))
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b):
        for i, (x, y) in enumerate(zip(a, b)):
            if not same_bits(x, y):
                return first_difference(x, y, "%s[%d]" % (path, i))
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape:
        bad = np.argwhere(bits(a) != bits(b))
        return "%s: %d of %d values differ, first at %s: %r against %r" % (path, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])
    return "%s: %r against %r" % (path, a, b)


def overruns():
    from lib import _native
    return _native.debug_set("pool_overruns", 0)


@functools.lru_cache(maxsize=None)
def selftest():
    """(ok, what was seen): the check mode fills what it hands out and finds a byte planted in a red zone"""
    from lib import _native
    lib, ctx = _native.load(), _native.Context.get()
    seen = {}
    quiesce()
    old = _native.debug_set("pool_check", -1)
    try:
        overruns()
        for byte in (0xFF, 0x7F):
            _native.debug_set("pool_check", byte)
            h = C.c_void_p()
            _native._check(lib.ics_img_create(ctx._h, 37, 45, C.byref(h)))
            img = _native.DeviceImage(h, ctx)
            seen["fill %#x" % byte] = np.unique(img.to_host().view(np.uint32)).tolist()
            img.close()
            seen["overruns after a clean block, fill %#x" % byte] = overruns()
        _native.debug_set("pool_selftest", 1)
        h = C.c_void_p()
        _native._check(lib.ics_img_create(ctx._h, 37, 45, C.byref(h)))
        _native.DeviceImage(h, ctx).close()
        seen["overruns after the planted byte"] = overruns()
        seen["pool_selftest afterwards"] = _native.debug_set("pool_selftest", 0)
    finally:
        _native.debug_set("pool_check", old)
        _native.debug_set("pool_selftest", 0)
    want = {"fill 0xff": [0xFFFFFFFF], "fill 0x7f": [0x7F7F7F7F], "overruns after a clean block, fill 0xff": 0,
            "overruns after a clean block, fill 0x7f": 0, "overruns after the planted byte": 1, "pool_selftest afterwards": 0}
    return seen == want, seen


def test_selftest_the_fill_is_seen_and_a_planted_byte_is_found():
    ok, seen = selftest()
    print(seen)
    assert ok, seen


@pytest.fixture(autouse=True)
def conclusive(request):
    """without a check mode that demonstrably fills and watches, nothing below says anything: skipped, not passed"""
    if request.node.name.startswith("test_selftest"):
        return
    ok, seen = selftest()
    if not ok:
        pytest.skip("inconclusive: the pool's self-test failed (%s)" % (seen,))


def nearest_measured(H, W, sizes):
    """(H, W) where the family measured its constants there, else the family's size nearest in area"""
    return (H, W) if (H, W) in sizes else min(sizes, key=lambda s: abs(np.log(s[0] * s[1] / float(H * W))))


def on_poison(debug_switch, run, reproducible=True):
    """run() -- which builds everything it uses and returns numpy results -- twice with the switch off, once per fill byte; gate (a)
    unless `reproducible` is False, no overrun in any case.  Returns ({fill byte: result}, the unpoisoned result, whether the two
    unpoisoned runs agreed)."""
    quiesce()
    overruns()
    ref = run(); quiesce()
    again = run(); quiesce()
    agreed = same_bits(ref, again)
    got = {}
    for byte in FILLS:
        debug_switch("pool_check", byte)
        got[byte] = run()
        quiesce()
    debug_switch("pool_check", -1)
    quiesce()
    # the context keeps its scratch between calls: one scratch call with the switch off returns the last check-mode block to the pool
    # (ctx_scratch, csrc/ics_host.h), so that it is verified before the counter is read
    from lib import _native
    _native.Context.get().conv2d_symm(np.zeros((2, 2)), np.ones((1, 1)))
    assert overruns() == 0, "a store past the end of a pool block (its line is on stderr)"
    if reproducible:
        assert agreed, "two unpoisoned runs differ: " + first_difference(ref, again)
        for byte, out in got.items():
            assert same_bits(out, ref), "fill %#x changes the result: %s" % (byte, first_difference(out, ref))
    return got, ref, agreed


# ---- resident image operators --------------------------------------------------------------------------------------------------------------
def _host(img):
    out = img.to_host()
    img.close()
    return out


def op_convolve(ctx, H, W):
    import test_gpu_img_filters as fm
    pic = fm.picture(H, W, seed=H * 7 + W)
    smax = float(np.abs(pic).max())
    kernels = {"gaussian15": fm.window_kernels()["gaussian15"], "random5x5": fm.random_kernel()}
    k17 = np.random.default_rng(8).random((1, 7)); k17 /= k17.sum()
    kernels["1x7"] = k17

    def run():
        from lib._native import DeviceImage
        img = DeviceImage.from_host(pic, ctx)
        return {name: _host(img.convolve(k)) for name, k in kernels.items()}

    def check(out):
        ref = {name: fm.per_channel(lambda ch: fm.uo.conv2d_symm(ch, k), pic) for name, k in kernels.items()}
        assert fm.worst(out["gaussian15"], ref["gaussian15"]) <= fm.blur_bound(kernels["gaussian15"], smax)
        kr = kernels["random5x5"]
        assert fm.worst(out["random5x5"], ref["random5x5"]) <= (kr.size + 2) * fm.EPS * np.abs(kr).sum() * smax
        assert fm.worst(out["1x7"], ref["1x7"]) <= (k17.size + 2) * fm.EPS * smax
    return run, check


def op_usm(ctx, H, W):
    import test_gpu_img_filters as fm
    pic = fm.picture(H, W, seed=H * 11 + W)
    smax = float(np.abs(pic).max())
    cases = [(15, 2.5, 0.8, "gauss"), (9, 4., -0.4, "bessel")]

    def run():
        from lib._native import DeviceImage
        img = DeviceImage.from_host(pic, ctx)
        return [_host(img.usm(*c)) for c in cases]

    def check(out):
        for o, (radius, strength, amount, method) in zip(out, cases):
            kern = {"gauss": fm.uo.gaussian_kernel, "bessel": fm.uo.kaiser_kernel}[method](radius, strength)
            ref = fm.per_channel(lambda ch: fm.uo.USM(ch, radius, strength, amount, method), pic)
            assert fm.worst(o, ref) <= fm.usm_bound(kern, amount, smax), (radius, amount, method)
    return run, check


def op_bilateral(ctx, H, W):
    import test_gpu_img_filters as fm
    pic = fm.bilateral_picture(H, W)
    params = [p for p in fm.BILATERAL_PARAMS if p[0] in (3, 10)]
    assert [p[0] for p in params] == [3, 10]
    rs = nearest_measured(H, W, fm.BILATERAL_SIZES)
    rpic = fm.bilateral_picture(*rs)

    def run():
        from lib._native import DeviceImage
        img, rimg = DeviceImage.from_host(pic, ctx), DeviceImage.from_host(rpic, ctx)
        return [_host(img.bilateral(*p)) for p in params], [_host(rimg.bilateral(*p)) for p in params]

    def check(out):
        for o, r, p in zip(out[0], out[1], params):
            for c in range(3):         # (test_bilateral_properties_are_exact) a weighted mean of the window stays inside the channel's range
                assert o[..., c].min() >= pic[..., c].min() and o[..., c].max() <= pic[..., c].max()
            err = fm.worst(r, fm.per_channel(lambda ch: fm.uo.bilateral_filter(ch, *p), rpic))
            assert err <= 4 * fm.F32_RESTATEMENT_ERROR[p], (rs, p, err)
    return run, check


def op_tv_denoise(ctx, H, W):
    import test_gpu_tv_denoise as tm
    pic = tm.tv_picture(H, W)
    assert 9 % tm.T                      # the blocked route's last launch runs a remainder
    weight, iterations = tm.PARAMS[1]
    assert iterations % tm.T             # ... and so does the measured set's
    rs = nearest_measured(H, W, tm.SIZES)
    rpic = tm.tv_picture(*rs)

    def run():
        from lib._native import DeviceImage
        img, rimg = DeviceImage.from_host(pic, ctx), DeviceImage.from_host(rpic, ctx)
        out = {(coupling, route): _host(img.tv_denoise(0.1, 9, coupling, route=route)) for coupling in tm.tvr.COUPLINGS for route in (0, 1, 2)}
        ref = {(coupling, route): _host(rimg.tv_denoise(weight, iterations, coupling, route=route)) for coupling in tm.tvr.COUPLINGS for route in (1, 2)}
        return out, ref

    def check(out):
        for coupling in tm.tvr.COUPLINGS:
            assert same_bits(out[0][coupling, 1], out[0][coupling, 2]) and same_bits(out[0][coupling, 0], out[0][coupling, 1]), coupling
            oracle = tm.tvr.tv_denoise(rpic, weight, iterations, coupling)
            for route in (1, 2):
                err = tm.worst(out[1][coupling, route], oracle)
                assert err <= 4 * tm.F32_RESTATEMENT_ERROR[coupling, weight, iterations], (rs, coupling, route, err)
    return run, check


def op_wavelet(ctx, H, W):
    import test_gpu_wavelet as wm
    pic = wm.wv_picture(H, W)
    sets = {"J3": (wm.MIXED[0][:3], wm.MIXED[1][:3], wm.MIXED[2]), "J8": wm.PARAMS["widest"] + (1.0,), "lift": wm.PARAMS["lift"] + (1.0,)}
    assert len(sets["J8"][0]) == 8 and (H, W) in wm.SIZES          # (the family measured its constants at all three sizes)

    def run():
        from lib._native import DeviceImage
        img = DeviceImage.from_host(pic, ctx)
        return {(name, coupling, route): _host(img.wavelet_equalize(g, t, res, coupling, route=route))
                for name, (g, t, res) in sets.items() for coupling in wm.wr.COUPLINGS for route in (0, 1, 2)}

    def check(out):
        for name in sets:
            for coupling in wm.wr.COUPLINGS:
                assert same_bits(out[name, coupling, 1], out[name, coupling, 2]) and same_bits(out[name, coupling, 0], out[name, coupling, 1])
        for name, measured in (("J8", "widest"), ("lift", "lift")):
            for coupling in wm.wr.COUPLINGS:
                err = wm.worst(out[name, coupling, 1], wm.oracle(H, W, measured, coupling))
                assert err <= 4 * wm.F32_RESTATEMENT_ERROR[coupling, measured], (measured, coupling, err)
    return run, check


def op_noise(ctx, H, W):
    import test_gpu_noise as nm
    pic = nm.ns_picture(H, W)

    def run():
        from lib._native import DeviceImage
        img = DeviceImage.from_host(pic, ctx)
        out = {(coupling, route): img.noise_estimate(coupling, route=route) for coupling in nm.nr.COUPLINGS for route in nm.ROUTES}
        img.close()
        return out

    def check(out):
        for (coupling, route), est in out.items():
            nm.check(est, pic, coupling)                # the median's bits against the float32 restatement
    return run, check


def op_despeckle(ctx, H, W):
    import test_gpu_despeckle as dm
    f = dm.frame(H, W, "salt")

    def run():
        from lib._native import DeviceImage
        img = DeviceImage.from_host(f, ctx)
        out = {}
        for radius in (1, 2):
            for coupling in dm.dr.COUPLINGS:
                for route in dm.ROUTES:
                    o, counts = img.despeckle(0.1, radius, coupling, route=route, count=True)
                    out[radius, coupling, route] = (_host(o), counts)
        return out

    def check(out):
        for (radius, coupling, route), (o, counts) in out.items():
            ref, ref_counts = dm.dr.despeckle(f, 0.1, radius, coupling)
            assert np.array_equal(dm.bits(o), dm.bits(ref)) and counts == ref_counts, (radius, coupling, route)
    return run, check


def op_guided(ctx, H, W):
    import test_gpu_guided as gm
    pic = gm.gf_picture(H, W)
    eps, detail = gm.EPS[0], gm.DETAILS[1]
    rs = nearest_measured(H, W, gm.SIZES)
    rpic = gm.gf_picture(*rs)

    def all_routes(img):
        return {(r, coupling, route): _host(img.guided_filter(r, eps, detail, coupling, route=route))
                for r in (4, 32) for coupling in gm.gr.COUPLINGS for route in gm.routes(r)}

    def run():
        from lib._native import DeviceImage
        out = all_routes(DeviceImage.from_host(pic, ctx))
        return out, (out if rs == (H, W) else all_routes(DeviceImage.from_host(rpic, ctx)))

    def check(out):
        assert gm.routes(4) == (0, 1, 2) and gm.routes(32) == (0, 1)
        for (r, coupling, route), o in out[0].items():
            assert same_bits(o, out[0][r, coupling, 0]), (r, coupling, route)
        for (r, coupling, route), o in out[1].items():
            err = gm.worst(o, gm.oracle(*rs, coupling, r, eps, detail))
            assert err <= 4 * gm.F32_RESTATEMENT_ERROR[coupling, r, eps], (rs, r, coupling, route, err)
    return run, check


def op_llf(ctx, H, W):
    import test_gpu_llf as lm
    pic = lm.llf_picture(H, W)
    args = lm.ARGS[0]
    rs = nearest_measured(H, W, lm.SIZES)
    rpic = lm.llf_picture(*rs)

    def all_routes(img):
        return {(J, K, coupling, route): _host(img.local_laplacian(*args, levels=J, samples=K, coupling=coupling, route=route))
                for J, K in ((3, 5), (6, 8)) for coupling in lm.lr.COUPLINGS for route in (0, 1, 2)}

    def run():
        from lib._native import DeviceImage
        out = all_routes(DeviceImage.from_host(pic, ctx))
        return out, (out if rs == (H, W) else all_routes(DeviceImage.from_host(rpic, ctx)))

    def check(out):
        for (J, K, coupling, route), o in out[0].items():
            assert same_bits(o, out[0][J, K, coupling, 0]), (J, K, coupling, route)
        for (J, K, coupling, route), o in out[1].items():
            err = lm.worst(o, lm.oracle(rs, args, J, K, coupling))
            assert err <= 4 * lm.F32_RESTATEMENT_ERROR[coupling, J, K], (rs, J, K, coupling, route, err)
    return run, check


def op_resize(ctx, H, W):
    import test_gpu_img_filters as fm
    pic = fm.picture(H, W, seed=H + 13 * W)
    shapes = [(max(2, (2 * H) // 3), max(2, (3 * W) // 5)), ((3 * H) // 2 + 1, (7 * W) // 4)]      # down, up

    def run():
        from lib._native import DeviceImage
        img = DeviceImage.from_host(pic, ctx)
        return [_host(img.resize(*s)) for s in shapes]

    def check(out):
        import resize_oracle as ro
        from test_driver import RESIZE_GATE
        for o, s in zip(out, shapes):      # (tests/test_driver.py::test_device_image_operations_match_numpy)
            assert o.shape == (*s, 3) and np.abs(o - ro.resize_scipy(pic, s).astype(np.float32)).max() < RESIZE_GATE, s
    return run, check


def op_exact(ctx, H, W):
    """pad_edge, crop, paste, copy, gamma and the 8- / 16-bit uploads, by the assertions of tests/test_driver.py"""
    import test_gpu_img_filters as fm
    a = fm.picture(H, W, seed=3 * H + W)
    rng = np.random.default_rng(H * W)
    px = {dt: rng.integers(0, top + 1, size=(H, W, 3)).astype(dt) for dt, top in ((np.uint8, 255), (np.uint16, 65535))}
    h2, w2 = max(1, H // 2), max(1, W // 2)

    def run():
        from lib._native import DeviceImage
        d = DeviceImage.from_host(a, ctx)
        out = {"pad": _host(d.pad_edge(2, 0, 1, 3)), "crop": _host(d.crop(H - h2, H, 1, 1 + w2)), "copy": _host(d.copy())}
        e = d.copy()
        piece = d.crop(0, h2, 0, w2)
        e.paste(H - h2, W - w2, piece)
        piece.close()
        out["paste"] = _host(e)
        g = d.copy(); g.gamma(2.0, 1 / 2.2)
        out["gamma"] = _host(g)
        g = d.copy(); g.gamma(0.5, 2.2, 65535, clip01=True)
        out["gamma_clip"] = _host(g)
        for dt, v in px.items():
            out[dt.__name__] = _host(DeviceImage.from_host(v, ctx))
        return out

    def check(out):
        from test_driver import GAMMA_CLIP_GATE, GAMMA_GATE
        assert np.array_equal(out["pad"], np.pad(a, ((2, 0), (1, 3), (0, 0)), mode="edge"))
        assert np.array_equal(out["crop"], a[H - h2:H, 1:1 + w2]) and np.array_equal(out["copy"], a)
        ref = a.copy(); ref[H - h2:, W - w2:] = a[:h2, :w2]
        assert np.array_equal(out["paste"], ref)
        assert np.abs(out["gamma"] - (a / np.float32(2.0)) ** np.float32(1 / 2.2)).max() < GAMMA_GATE
        assert np.abs(out["gamma_clip"] - np.clip(a / np.float32(0.5), 0, 1) ** np.float32(2.2) * np.float32(65535)).max() < GAMMA_CLIP_GATE
        for dt, v in px.items():
            assert np.array_equal(out[dt.__name__], v.astype(np.float32))
    return run, check


def op_float64(ctx, H, W):
    """the stand-alone float64 operators on host arrays (the context's scratch among their buffers), by the gates of tests/test_utils.py
    and tests/test_resize.py"""
    import test_gpu_img_filters as fm
    pic = fm.picture(H, W, seed=5 * H + W)
    ch = pic[..., 0].astype(np.float64)
    kern = fm.window_kernels()["gaussian15"]
    k2 = np.random.default_rng(4).random((9, 7)); k2 /= k2.sum()
    dst = (max(2, (2 * H) // 3), (7 * W) // 4)

    def run():
        out = {"tv": [ctx.tv(pic, eps, order, norm) for eps in (1e-2, 1e-6) for order, norm in ((2, 1), (1, 2))],
               "conv_sep": ctx.conv2d_symm(ch, kern), "conv_2d": ctx.conv2d_symm(ch, k2), "usm": ctx.usm(ch, kern, 0.8),
               "bilateral": ctx.bilateral(ch, 3, 0.2, 1.5)}
        if H >= 2 and W >= 2:
            out["resize"] = ctx.resize_bicubic(pic.astype(np.float64), dst)
        return out

    def check(out):
        import resize_oracle as ro
        import rl_mm_oracle as orc
        from scipy.signal import convolve2d
        from test_resize import EXTREME_GATE
        from test_utils import BILATERAL_RTOL, CONV_ATOL, CONV_RTOL, TV_NORM2_RTOL, USM_ATOL
        i = 0
        for eps in (1e-2, 1e-6):
            for order, norm in ((2, 1), (1, 2)):
                o, div = out["tv"][i]; i += 1
                ro_, rd = orc.TV(pic, H, W, eps, order, norm)
                assert np.array_equal(div, rd)
                if norm == 1:
                    assert np.array_equal(o, ro_)
                else:
                    np.testing.assert_allclose(o, ro_, rtol=TV_NORM2_RTOL, atol=0)
        ref = convolve2d(ch, kern, mode="same", boundary="symm")
        np.testing.assert_allclose(out["conv_sep"], ref, rtol=CONV_RTOL, atol=CONV_ATOL)
        np.testing.assert_allclose(out["conv_2d"], convolve2d(ch, k2, mode="same", boundary="symm"), rtol=CONV_RTOL, atol=CONV_ATOL)
        np.testing.assert_allclose(out["usm"], ch + (ch - ref) * 0.8, rtol=CONV_RTOL, atol=USM_ATOL)
        np.testing.assert_allclose(out["bilateral"], fm.uo.bilateral_filter(ch, 3, 0.2, 1.5), rtol=BILATERAL_RTOL)
        if "resize" in out:
            assert np.abs(out["resize"] - ro.resize_scipy(pic.astype(np.float64), dst)).max() < EXTREME_GATE
    return run, check


OPERATORS = {"convolve": op_convolve, "usm": op_usm, "bilateral": op_bilateral, "tv_denoise": op_tv_denoise, "wavelet_equalize": op_wavelet,
             "noise_estimate": op_noise, "despeckle": op_despeckle, "guided_filter": op_guided, "local_laplacian": op_llf, "resize": op_resize,
             "exact": op_exact, "float64": op_float64}


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("name", list(OPERATORS))
def test_image_operator_on_poisoned_blocks(ctx, debug_switch, name, H, W):
    run, check = OPERATORS[name](ctx, H, W)
    got, ref, _ = on_poison(debug_switch, run)                # gate (a), no overrun
    check(got[FILLS[0]])                                       # gate (b); by gate (a) the three poisoned results are one and the same


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
def whole_run(c):
    """the case through the product path (as run_device of tests/test_gpu_route_matrix.py, with the printed lines kept): everything a
    caller sees"""
    from lib import _native as nv
    from lib import deconvolution as dc
    image, u0, psf0 = rc.make_data(c)
    if c.fuse:                             # (an RLJob of its own, params.fuse set: nothing is printed)
        u, psf, psf_caller, img, st, lines, route = rm.run_device(c, image, u0, psf0)
    else:
        with rc.switches_set(c):
            job = dc._get_job(c.M, c.N, c.MK)
            route = rc.route_tuple(job.describe(rc.params_of(nv, c)))
            img, u, psf_caller = image.copy(), u0.copy(), psf0.copy()
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                dc.richardson_lucy_MM(img, u, psf_caller, *rm._args(c), blind=c.blind, correlation=bool(c.correlation), tv_mode=c.tv_mode,
                                      conv=c.conv, flags=c.flags)
            st = dc.richardson_lucy_MM.last
            psf = job.download()[1]
            lines = buf.getvalue().splitlines()
    n = st.trace_len
    traces = [np.array(getattr(st, "trace_" + f)[:n], np.float32) for f in ("M_r", "Hu", "varu", "dof_min", "dof_max")]
    return {"u": u, "psf": psf, "psf_caller": psf_caller, "image": img, "iterations": st.iterations_done, "stopped": int(st.stopped),
            "has_nan": int(st.has_nan), "lines": lines, "traces": traces, "route": route}


def check_whole(debug_switch, c, route_char=None, tid=None):
    reproducible = (tid or c.id) not in NOT_REPRODUCIBLE
    _, _, agreed = on_poison(debug_switch, lambda: whole_run(c), reproducible)
    if not reproducible:
        assert not agreed, "%s is on NOT_REPRODUCIBLE but two unpoisoned runs agree bit for bit: take it off the list" % (tid or c.id)
    for byte in FILLS if not reproducible else FILLS[:1]:      # gate (b); reproducible routes: the three poisoned runs are one and the same
        quiesce()
        debug_switch("pool_check", byte)
        rm.check_case(c, route_char)
        quiesce()
        debug_switch("pool_check", -1)
    assert overruns() == 0


_PICK = sorted(rc.cheapest_per_route().items())


@pytest.mark.parametrize("key,c", _PICK, ids=["tv%d-route-%s-%s" % (k[0], k[1], c.id) for k, c in _PICK])
def test_whole_run_on_poisoned_blocks(debug_switch, key, c):
    check_whole(debug_switch, c, key[1])


# the buffers no route implies
EXTRA = [
    # overlapped statistics everywhere (overlap = 2): the second residual frame e2, and psf_bak of a blind run
    rc.Case("overlap2-nb", 129, 191, 7, False, conv=2, win=(10, 120, 20, 170), seed=11, switches=(("overlap", 2),)),
    rc.Case("overlap2-bl", 129, 191, 7, True, conv=2, win=(10, 120, 20, 170), seed=12, switches=(("overlap", 2),)),
    rc.Case("overlap2-small-bl", 97, 129, 9, True, win=(5, 90, 10, 120), seed=13, switches=(("overlap", 2),)),
    # one long-line window (a side above 4096 px): z as [3][H][Px] rows and their transpose, the full twiddle tables of both axes
    rc.Case("long-line", 4300, 96, 5, False, win=(0, 4300, 0, 96), seed=14),
    # PSF 65 as tap blocks on the matrix cores (blk_conv, blk_corr, blk_scr, blk_negf, blk_red, psf_work)
    rc.Case("blocks-65", 120, 110, 65, True, win=(10, 110, 10, 100), seed=15),
    # PSF 71 (one tile per PSF) and 97 (tap blocks on the tiles), blind
    rc.Case("tiles-71", 120, 110, 71, True, conv=3, win=(10, 110, 10, 100), seed=16),
    rc.Case("tiles-97", 120, 110, 97, True, conv=3, win=(10, 110, 10, 100), seed=17),
]


# the route each of them must take (legend character of tests/golden/route_table.json: conv family, fp16 split, gradient family, ...),
# so that a change of the routing thresholds cannot move a case off the buffers it is here for
EXTRA_ROUTES = {"overlap2-nb": "1", "overlap2-bl": "8", "overlap2-small-bl": "5", "long-line": "c", "blocks-65": "i", "tiles-71": "a",
                "tiles-97": "b"}


@pytest.mark.parametrize("c", EXTRA, ids=lambda c: c.id)
def test_whole_run_with_the_buffers_no_route_implies(debug_switch, c):
    leg = {v: k for k, v in rc.legend().items()}
    family = leg[EXTRA_ROUTES[c.id]][0]
    assert family == {"overlap2-nb": 1, "overlap2-bl": 1, "overlap2-small-bl": 6, "long-line": 1, "blocks-65": 2, "tiles-71": 5, "tiles-97": 5}[c.id]
    if c.id.startswith("overlap2"):
        # ics_rl_describe does not report the second stream; resolve_route (csrc/ics_route.hip) takes it for overlap = 2 unless the run
        # fuses, steps the image (tv_mode 1), has an empty window or a single iteration
        assert c.switch("overlap") == 2 and not c.fuse and c.tv_mode != 1 and c.iters >= 2 and c.win[1] > c.win[0] and c.win[3] > c.win[2]
    if c.id == "long-line":
        assert max(c.win[1] - c.win[0], c.win[3] - c.win[2]) > 4096         # ensure_window's long-line path
    check_whole(debug_switch, c, EXTRA_ROUTES[c.id])                         # (check_case asserts the route the job describes)


def test_window_then_empty_window_then_another_window_on_one_job(debug_switch):
    """the stop test's z, tw and weights are dropped and allocated again when the window changes (ensure_window): three calls on ONE
    cached job, the last one through check_case"""
    from lib import deconvolution as dc
    M, N, MK = 130, 150, 9
    wins = [(10, 100, 20, 120), (40, 40, 20, 120), (3, 127, 5, 70)]
    cs = [rc.Case("win%d" % i, M, N, MK, True, conv=2, win=w, seed=21) for i, w in enumerate(wins)]

    def run():
        out = []
        for c in cs:                       # (the job of this shape stays cached between the three)
            out.append(whole_run(c))
        assert len(dc._job_cache) == 1
        # the empty window: NaN statistics, printed as the reference prints them (nan, no ZeroDivisionError from the closing line)
        assert np.isnan(out[1]["traces"][0]).all() and any(l.startswith("Stats : autocovariance = nan") for l in out[1]["lines"]), out[1]["lines"]
        return out

    on_poison(debug_switch, run)
    for byte in FILLS[:1]:
        quiesce()
        debug_switch("pool_check", byte)
        whole_run(cs[0]); whole_run(cs[1])
        rm.check_case(cs[2])
        quiesce()
        debug_switch("pool_check", -1)
    assert overruns() == 0


def test_two_row_bands_blind(debug_switch):
    """lib.banded.richardson_lucy_MM_banded(bands=2), blind: a job per band and the statistics job, against the single job by the gate of
    tests/test_banded.py::test_blind_bands_match_one_job"""
    import rl_mm_oracle as orc
    import test_banded as tb
    M, N, MK = 300, 260, 15
    case = orc.synth_case(M, N, MK, seed=9, blind=True)
    win = (110, 191, 60, 201)

    def run():
        u, p, log, st = tb.run_banded(case, M, N, MK, win, 0.0, 2, True, 0, 2)
        return {"u": u, "psf": p, "log": log, "iterations": st.iterations_done, "M_r": float(st.M_r), "Hu": float(st.Hu)}

    tid = "bands2-bl"
    got, ref, agreed = on_poison(debug_switch, run, tid not in NOT_REPRODUCIBLE)
    assert agreed or tid in NOT_REPRODUCIBLE
    u1, p1, _, st1 = tb.run_single(case, M, N, MK, win, 0.0, 2, True, 0, flags=1)
    for byte in FILLS:
        o = got[byte]
        assert o["iterations"] == st1.iterations_done
        assert tb.rel_err(o["u"], u1) < tb.BLIND_BANDS_GATE and tb.rel_err(o["psf"], p1) < tb.BLIND_BANDS_GATE
        assert abs(o["M_r"] - st1.M_r) <= tb.BLIND_BANDS_MR_RTOL * abs(st1.M_r) and abs(o["Hu"] - st1.Hu) <= tb.BLIND_BANDS_HU_RTOL * abs(st1.Hu)


def test_deblur_module_resident_with_every_filter(debug_switch, capsys):
    """deblur_module(device_resident=True, pyramid=True) on the SMALL picture of tests/test_driver.py with despeckle, denoise, clarity,
    local_contrast, detail and sharpen set: a job and a handful of images per pyramid level and phase, the production allocation
    pattern.  No test pins the two drivers against each other, or either against a reference, with all six steps set, so there is NO
    gate (b) here: the resident run and the host-frame run (device_resident=False) are each held to gate (a) -- their own unpoisoned run,
    bit for bit, printed lines included -- and to pool_overruns == 0; the resident output also to what tests/test_driver.py asserts of
    every output (shape, finite, 16-bit range, a normalised non-negative PSF).  The steps themselves have their gate (b) above."""
    import deconvolve as dv
    import rl_mm_oracle as orc
    from test_driver import PSF_SUM_ATOL, SMALL
    K = SMALL["K"]
    case = orc.synth_case(*SMALL["shape"], K, seed=2)
    pic = np.clip(case["image"] ** 2.2 * 255, 0, 255).astype(np.uint8)
    kw = dict(mask=SMALL["mask"], mask_size=SMALL["mask_size"], display=False, iterations=SMALL["iterations"], pyramid=True, save=False,
              despeckle=("auto",), denoise=(0.05, 20), clarity=(0.2, 1.8), local_contrast=((1.5, 1.2, 1.0), "auto"), detail=(4, 1e-2, 1.5),
              sharpen=(9, 4., 0.5))

    def run(resident):
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            out, psf = dv.deblur_module(pic, "p", ".", K, device_resident=resident, **kw)
        lines = [l for l in buf.getvalue().splitlines() if not l.startswith("'deblur_module'") and "sec" not in l]
        return {"out": np.asarray(out), "psf": np.asarray(psf), "lines": lines}

    got, ref, _ = on_poison(debug_switch, lambda: run(True))
    for o in got.values():
        assert o["out"].shape == (*SMALL["shape"], 3) and np.isfinite(o["out"]).all() and o["out"].min() >= 0 and o["out"].max() <= 65535
        assert np.all(o["psf"] >= 0) and np.allclose(o["psf"].sum(axis=(0, 1)), 1, atol=PSF_SUM_ATOL)
    on_poison(debug_switch, lambda: run(False))
