"""GPU: DeviceImage.shock and DeviceImage.edge_mask (csrc/ics_img_edges.hip) against the float32 evaluation of the specification
(tests/edges_ref.py), bit for bit, on both routes and both couplings.  Shapes: a frame smaller than anything (5 x 7), one 32 x 32
tile of the blocked route and one pixel / three pixels over, a frame that is no multiple of anything, tile-exact 64 x 96 and one over,
and a frame of three by five tiles whose last ones are partial.  Steps: 1, 4 (one launch of the blocked route), 5 (a remainder
launch) and 9 (two full launches and a remainder, both ping-pong frames in use).  A wrong halo, clamp or region of the blocked route
shows at a tile edge of exactly these shapes.

The edge mask's kernels are persistent workgroups (at most cus x 1, x 4 or x 8) over 4 x 64 pixel tiles and units of 1024 or 256 keys: on
these shapes and 256 CUs every workgroup makes one trip.  70 x 150 and 301 x 287 with the max_wgs switch at 2 and 1, and a frame past
the launcher's own caps (tests/trips_ref.py past_the_caps: 1030 x 1100), make them add further tiles to a live LDS histogram and carry
their kept counts from trip to trip."""
import functools
import gc

import numpy as np
import pytest

import edges_ref as er
import trips_ref as tr

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (32, 32), (33, 35), (40, 52), (64, 96), (65, 97), (70, 150)]
STEPS = [1, 4, 5, 9]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def ref_shock(shape, steps, coupling):
    out = er.shock(er.frame(shape), steps, er.SHOCK[1], er.SHOCK[2], coupling, np.float32)
    out.setflags(write=False)
    return out


def dev_shock(f, steps, coupling, route, dt=er.SHOCK[1], flat=er.SHOCK[2]):
    from lib import _native
    d = _native.DeviceImage.from_host(f)
    try:
        o = d.shock(steps, dt, flat, coupling, route)
        try:
            return o.to_host()
        finally:
            o.close()
    finally:
        d.close()


def dev_mask(f, per_sector, coupling, route):
    from lib import _native
    d = _native.DeviceImage.from_host(f)
    try:
        m = d.edge_mask(per_sector, coupling, route)
        try:
            return m.mask.to_host(), m.threshold, m.kept
        finally:
            m.mask.close()
    finally:
        d.close()


@pytest.mark.parametrize("coupling", er.COUPLINGS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_shock_gives_the_bits_of_the_float32_specification_on_both_routes(shape, steps, coupling):
    f = er.frame(shape)
    ref = ref_shock(shape, steps, coupling)
    assert not np.array_equal(bits(ref), bits(f))                       # the filter moves this frame
    for route in (1, 2):
        out = dev_shock(f, steps, coupling, route)
        assert out.shape == ref.shape and out.dtype == np.float32
        bad = bits(out) != bits(ref)
        assert not bad.any(), "route %d: %d values differ, first at %s, max |diff| %.3g" % (
            route, bad.sum(), np.argwhere(bad)[0], np.abs(out.astype(np.float64) - ref).max())
    assert np.array_equal(bits(dev_shock(f, steps, coupling, 0)), bits(ref))


def test_no_step_is_a_copy_and_other_parameters_match_too():
    f = er.frame((40, 52))
    assert np.array_equal(bits(dev_shock(f, 0, "vector", 0)), bits(f))
    for dt, flat in ((0.25, 0.05), (-0.3, 0.002)):                      # (a negative dt blurs: the steer's sign matters)
        for coupling in er.COUPLINGS:
            ref = er.shock(f, 3, dt, flat, coupling, np.float32)
            for route in (1, 2):
                assert np.array_equal(bits(dev_shock(f, 3, coupling, route, dt, flat)), bits(ref))


def per_sector_cases(shape):
    n = shape[0] * shape[1]
    return [1, max(2, n // 16), n + 5]                                   # the single largest, a share, more than any sector holds


@pytest.mark.parametrize("coupling", er.COUPLINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_edge_mask_of_the_devices_own_shock_frame_matches_the_specification(shape, coupling):
    p = dev_shock(er.frame(shape), 4, coupling, 0)
    for per_sector in per_sector_cases(shape):
        mask, t, kept = er.edge_mask(p, per_sector, coupling, np.float32)
        for route in (1, 2, 0):
            m, th, k = dev_mask(p, per_sector, coupling, route)
            assert m.dtype == bool and m.shape == mask.shape
            assert np.array_equal(bits(np.asarray(th, np.float32)), bits(np.asarray(t, np.float32))), (route, per_sector, th, t)
            assert k == kept and np.array_equal(m, mask), (route, per_sector, k, kept)


def assert_mask(got, want, what):
    """(mask, threshold, kept) of the device against the specification's or another run's: every bit"""
    assert got[0].dtype == bool and got[0].shape == want[0].shape, what
    assert np.array_equal(bits(np.asarray(got[1], np.float32)), bits(np.asarray(want[1], np.float32))), (what, got[1], want[1])
    assert np.array_equal(np.asarray(got[2]), np.asarray(want[2])) and np.array_equal(got[0], want[0]), (what, got[2], want[2])


@pytest.mark.parametrize("coupling", er.COUPLINGS)
@pytest.mark.parametrize("shape", [(70, 150), (301, 287)])
def test_edge_mask_by_two_workgroups_and_by_one_that_walk_every_tile(debug_switch, shape, coupling):
    """the max_wgs switch caps every persistent grid of the launcher: with 2 and with 1 workgroups each walks many tiles and key units
    (54 and 11 on 70 x 150; 380, 85 and 338 on the ragged 301 x 287), adds them to a live LDS histogram and carries its kept count from
    trip to trip.  The counts are integers: whoever walks the tiles, the bits are those of the specification and of the uncapped run."""
    p = dev_shock(er.frame(shape), 4, coupling, 0)
    for route in (1, 2):
        assert all(units > 2 for units, _ in tr.edge_mask_grids(*shape, coupling, route).values())
    for per_sector in per_sector_cases(shape):
        want = er.edge_mask(p, per_sector, coupling, np.float32)
        full = {route: dev_mask(p, per_sector, coupling, route) for route in (1, 2, 0)}
        for cap in (2, 1):
            debug_switch("max_wgs", cap)
            capped = {route: dev_mask(p, per_sector, coupling, route) for route in (1, 2, 0)}
            debug_switch("max_wgs", 0)
            for route in (1, 2, 0):
                what = "route %d, per_sector %d, max_wgs %d" % (route, per_sector, cap)
                assert_mask(capped[route], want, what)
                assert_mask(capped[route], full[route], what + " against the uncapped run")


@pytest.mark.parametrize("coupling", er.COUPLINGS)
def test_edge_mask_on_a_frame_with_more_units_than_workgroups(ctx, coupling):
    """no switch: a frame large enough for the launcher's own caps (cus x 1 "channel", cus x 4 "vector" for the count passes, cus x 8
    for the mask kernels), 1030 x 1100 on 256 CUs, no side a multiple of the 4 x 64 tile.  Every workgroup of every kernel takes a
    second tile or key unit; asserted from the device's CU count, so that a larger device fails here instead of testing nothing."""
    shape = tr.past_the_caps(ctx.compute_units)
    assert shape[0] % 4 and shape[1] % 64
    for route in (1, 2):
        for kernel, (units, cap) in tr.edge_mask_grids(*shape, coupling, route, ctx.compute_units).items():
            print("edge mask %s %d x %d on %d CUs, %s: %d units for %d workgroups" % ((coupling,) + shape + (ctx.compute_units, kernel, units, cap)))
            assert units > cap, (kernel, units, cap)
    with np.errstate(over="ignore"):                                     # (a sigmoid far from its edge: exp overflows to inf, the term is 0)
        f = er.frame(shape)
    p = dev_shock(f, 4, coupling, 0)
    assert not np.array_equal(bits(p), bits(f))
    for per_sector in per_sector_cases(shape):
        want = er.edge_mask(p, per_sector, coupling, np.float32)
        for route in (1, 2, 0):
            assert_mask(dev_mask(p, per_sector, coupling, route), want, "route %d, per_sector %d" % (route, per_sector))


def test_one_orientation_few_in_a_sector_and_ties_at_the_threshold():
    # vertical edges only (sector 0): steps of three heights along x, constant along y
    row = np.cumsum(np.array([0, 0.125, 0, 0.25, 0, 0.125, 0.5, 0, 0.25, 0.125, 0, 0], np.float32)).astype(np.float32)
    f = np.repeat(np.repeat(row[None, :, None], 6, axis=0), 3, axis=2) * np.float32(0.25) + np.float32(0.125)
    g, sec = er.gradient_keys(f, "vector", np.float32)
    assert set(np.unique(sec)) == {0, 4}
    for per_sector in (1, 6, 7, 13, 1000):                              # 6 pixels tie at every height: the threshold takes whole groups
        mask, t, kept = er.edge_mask(f, per_sector, "vector", np.float32)
        assert kept % 6 == 0 and kept >= min(per_sector, 36)
        for route in (1, 2):
            m, th, k = dev_mask(f, per_sector, "vector", route)
            assert np.float32(th) == t and k == kept and np.array_equal(m, mask)
    # a faint dent beside many vertical steps: sector 1 holds a single pixel, and its gradient is the threshold
    f2 = f.copy()
    f2[0, 10, :] -= np.float32(2.0 ** -10)
    g, sec = er.gradient_keys(f2, "vector", np.float32)
    assert (sec == 1).sum() == 1
    for per_sector in (1, 4):
        mask, t, kept = er.edge_mask(f2, per_sector, "vector", np.float32)
        for coupling in er.COUPLINGS:
            want = er.edge_mask(f2, per_sector, coupling, np.float32)
            for route in (1, 2):
                m, th, k = dev_mask(f2, per_sector, coupling, route)
                assert np.array_equal(bits(np.asarray(th, np.float32)), bits(np.asarray(want[1], np.float32))) and k == want[2] and np.array_equal(m, want[0])


def test_two_runs_give_identical_bits_and_the_source_is_untouched():
    from lib import _native
    f = er.frame((70, 150))
    d = _native.DeviceImage.from_host(f)
    a, b = d.shock(9, route=2), d.shock(9, route=2)
    ha, hb = a.to_host(), b.to_host()
    m1, m2 = a.edge_mask(300), a.edge_mask(300)
    same = np.array_equal(m1.mask.to_host(), m2.mask.to_host()) and m1.threshold == m2.threshold and m1.kept == m2.kept
    assert m1.mask.shape == (70, 150)
    back, shocked = d.to_host(), a.to_host()
    for o in (a, b, d, m1.mask, m2.mask):
        o.close()
    assert np.array_equal(bits(ha), bits(hb)) and same
    assert np.array_equal(bits(back), bits(f)) and np.array_equal(bits(shocked), bits(ha))


def test_on_poisoned_red_zoned_pool_blocks(debug_switch):
    """pool check mode (csrc/ics_pool.h): every block the calls take is filled with 0xFF and its red zone verified when it goes back: a
    read of a ping-pong frame, key or histogram word nobody wrote would change the result, a store past a block's end would be counted"""
    from lib import _native
    from lib import deconvolution as dc
    f = er.frame((70, 150))
    for coupling in er.COUPLINGS:
        for route in (1, 2):
            clean = dev_shock(f, 9, coupling, route)
            cm = dev_mask(clean, 200, coupling, route)
            dc._drop_jobs(); gc.collect()
            _native.debug_set("pool_overruns", 0)
            debug_switch("pool_check", 0xFF)
            poisoned = dev_shock(f, 9, coupling, route)
            pm = dev_mask(clean, 200, coupling, route)
            gc.collect()
            debug_switch("pool_check", -1)
            gc.collect()
            assert _native.debug_set("pool_overruns", 0) == 0
            assert np.array_equal(bits(poisoned), bits(clean))
            assert np.array_equal(pm[0], cm[0]) and np.array_equal(pm[1], cm[1]) and pm[2] == cm[2]


def test_refusals():
    from lib import _native
    f = er.frame((40, 52))
    d = _native.DeviceImage.from_host(f)
    flat = _native.DeviceImage.from_host(np.full((12, 9, 3), 0.25, np.float32))
    one = f.copy()
    one[..., 1] = 0.5                                                    # a constant channel: refused per channel, fine as a vector
    dc = _native.DeviceImage.from_host(one)
    try:
        for kw in (dict(iterations=-1), dict(iterations=1.5), dict(dt=np.nan), dict(flat=0.0), dict(flat=-1.0), dict(flat=np.inf),
                   dict(coupling="rgb"), dict(route=3)):
            with pytest.raises(ValueError):
                d.shock(**kw)
        for args in ((0,), (-3,), (2.5,), (4, "rgb"), (4, "vector", 5)):
            with pytest.raises(ValueError):
                d.edge_mask(*args)
        with pytest.raises(ValueError, match="no gradients to select"):
            flat.edge_mask(4)
        with pytest.raises(ValueError, match="no gradients to select"):
            dc.edge_mask(4, "channel")
        m = dc.edge_mask(4, "vector")
        assert m.kept >= 4
        m.mask.close()
        # ... and by the native entries themselves
        import ctypes as C
        h = C.c_void_p()
        lib = _native.load()
        assert lib.ics_img_shock(d._h, -1, 0.4, 0.01, 1, 0, C.byref(h)) == _native.ICS_EINVAL and not h.value
        assert lib.ics_img_shock(d._h, 1, 0.4, 0.0, 1, 0, C.byref(h)) == _native.ICS_EINVAL and not h.value
        t, k = (C.c_float * 3)(), (C.c_uint * 3)()
        assert lib.ics_img_edge_mask(d._h, 0, 1, 0, C.byref(h), t, k) == _native.ICS_EINVAL and not h.value
        assert lib.ics_img_edge_mask(flat._h, 3, 1, 1, C.byref(h), t, k) == _native.ICS_OK and h.value      # nothing to select: a NaN threshold,
        m = _native.DeviceMask(h, d.ctx)                                                                       # an empty mask, a count of 0
        assert np.isnan(t[0]) and k[0] == 0 and not m.to_host().any()
        m.close()
    finally:
        d.close(); flat.close(); dc.close()
