"""CPU: the specification of the edge predictor itself (tests/edges_ref.py): one shock step in float32 against float64, the steer's
continuity, and the sector and select rule on hand-built frames."""
import numpy as np
import pytest

import edges_ref as er

SHAPES = [(5, 7), (32, 32), (33, 35), (40, 52), (64, 96), (65, 97), (70, 150)]


@pytest.mark.parametrize("coupling", er.COUPLINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_one_shock_step_in_float32_is_within_the_gate_of_float64_everywhere(shape, coupling):
    f = er.frame(shape)
    a, b = er.shock_step(f, er.SHOCK[1], er.SHOCK[2], coupling, np.float32), er.shock_step(f, er.SHOCK[1], er.SHOCK[2], coupling, np.float64)
    assert a.dtype == np.float32 and b.dtype == np.float64 and a.shape == b.shape == f.shape
    err = np.abs(a.astype(np.float64) - b) / np.maximum(1.0, np.abs(b))
    outside = float((err > er.ONE_STEP_GATE).mean())
    print("one shock step %s %s: max error %.3g, share outside %.3g" % (shape, coupling, err.max(), outside))
    assert outside == 0.0
    assert np.abs(b - f).max() > 1e-3                                   # the step does move this frame


def test_the_steer_is_continuous_and_saturates():
    f = er.frame((40, 52))
    s = er.steer(f, er.SHOCK[2], "vector")
    assert s.shape == (40, 52) and np.abs(s).max() == 1.0 and ((np.abs(s) > 0) & (np.abs(s) < 1)).any()
    # a perturbation of the frame far below float32's rounding moves s by no more than its Lipschitz bound (16 / flat per unit of Y):
    # a hard sign would jump by 2 at some pixel
    g = f.astype(np.float64) + 1e-9 * np.random.default_rng(0).standard_normal(f.shape)
    assert np.abs(er.steer(g, er.SHOCK[2], "vector") - s).max() <= 16 / er.SHOCK[2] * 1e-8
    assert er.steer(f, er.SHOCK[2], "channel").shape == (40, 52, 3)


def test_a_flat_frame_and_a_linear_ramp_stay_where_they_are():
    flat = np.full((9, 11, 3), 0.3, np.float32)
    assert np.array_equal(er.shock(flat, 4, dtype=np.float32), flat)
    ramp = np.repeat((np.arange(16, dtype=np.float32) / 32)[None, :, None], 8, axis=0).repeat(3, axis=2)
    out = er.shock(ramp, 1, dtype=np.float32)
    assert np.array_equal(out[:, 3:-3], ramp[:, 3:-3])                   # no curvature, no motion (the clamped ends have some)


def test_shock_steepens_a_blurred_step():
    x = np.arange(40, dtype=np.float64)
    row = 0.2 + 0.6 / (1 + np.exp(-(x - 19.5) / 3.0))
    f = np.repeat(np.repeat(row[None, :, None], 6, axis=0), 3, axis=2).astype(np.float32)
    out = er.shock(f, 8, dtype=np.float32)
    assert np.abs(np.diff(out[3, :, 0])).max() > 1.5 * np.abs(np.diff(f[3, :, 0])).max()
    assert out.min() >= f.min() - 1e-6 and out.max() <= f.max() + 1e-6  # minmod differences: no overshoot


def steps_frame():
    row = np.cumsum(np.array([0, 0.125, 0, 0.25, 0, 0.125, 0.5, 0, 0.25, 0.125, 0, 0], np.float32)).astype(np.float32)
    return np.repeat(np.repeat(row[None, :, None], 6, axis=0), 3, axis=2) * np.float32(0.25) + np.float32(0.125)


def test_one_orientation_only_and_ties_at_the_threshold():
    f = steps_frame()                                                   # vertical edges: 3 columns of height 1, 2 of height 2, 1 of height 4
    g, sec = er.gradient_keys(f, "vector", np.float32)
    assert set(np.unique(sec)) == {0, 4} and (sec == 0).sum() == 36
    heights = np.unique(g[sec == 0])
    assert heights.size == 3
    for per_sector, kept in ((1, 6), (6, 6), (7, 18), (18, 18), (19, 36), (36, 36), (1000, 36)):   # ties: whole groups of equal gradients
        mask, t, k = er.edge_mask(f, per_sector, "vector", np.float32)
        assert k == kept and mask.sum() == kept and t == heights[{6: 2, 18: 1, 36: 0}[kept]]
        assert not mask[:, -1].any()
    # the same frame turned: sector 2
    g, sec = er.gradient_keys(np.ascontiguousarray(f.transpose(1, 0, 2)), "vector", np.float32)
    assert set(np.unique(sec)) == {2, 4}


def test_a_sector_with_fewer_than_per_sector_sets_the_threshold_by_its_smallest():
    f = steps_frame()
    f[0, 10, :] -= np.float32(2.0 ** -10)                                # a faint dent in the flat part: one pixel with gx = gy > 0, sector 1
    g, sec = er.gradient_keys(f, "vector", np.float32)
    assert (sec[0] == 1).sum() == 1 and sec[0, 0, 10] == 1 and sec[0, 0, 9] == 0 and (sec[0] == 2).sum() == 0 and (sec[0] == 3).sum() == 0
    mask, t, kept = er.edge_mask(f, 4, "vector", np.float32)
    assert t == g[0, 0, 10] < g[0][sec[0] == 0].max()                     # sector 1 keeps the one it has: its gradient is the threshold
    assert kept == int((g >= t).sum()) and mask[0, 10] and not mask[0, 9]  # ... and the fainter pixel beside it (sector 0) stays out
    assert er.edge_mask(f, 1, "vector", np.float32)[1] == t


def test_diagonal_sectors_by_the_sign_of_the_product():
    y, x = np.mgrid[0:12, 0:12].astype(np.float32)
    plane = lambda a, b: np.repeat(((a * x + b * y) / np.float32(64) + np.float32(0.5))[..., None], 3, axis=2)
    for a, b, want in ((1, 1, 1), (-1, -1, 1), (1, -1, 3), (-1, 1, 3), (4, 1, 0), (-4, 1, 0), (1, 4, 2), (1, -4, 2), (2, 1, 1), (2, -1, 3)):
        sec = er.gradient_keys(plane(a, b), "vector", np.float32)[1][0, :-1, :-1]
        assert (sec == want).all(), (a, b, want)


def test_a_constant_frame_is_refused():
    with pytest.raises(ValueError, match="no gradients to select"):
        er.edge_mask(np.full((8, 9, 3), 0.5, np.float32), 3)
    one = er.frame((8, 9))
    one[..., 2] = 0.25
    with pytest.raises(ValueError, match="no gradients to select"):
        er.edge_mask(one, 3, "channel")
    assert er.edge_mask(one, 3, "vector")[2] >= 3


def test_channel_coupling_selects_every_channel_on_its_own():
    f = er.frame((33, 35))
    mask, t, kept = er.edge_mask(f, 40, "channel", np.float32)
    assert mask.shape == (33, 35, 3) and t.shape == (3,) and len(kept) == 3
    for c in range(3):
        solo = np.repeat(f[..., c:c + 1], 3, axis=2)
        m, tc, k = er.edge_mask(solo, 40, "channel", np.float32)
        assert np.array_equal(m[..., 0], mask[..., c]) and tc[0] == t[c] and k[0] == kept[c]


@pytest.mark.parametrize("coupling", er.COUPLINGS)
def test_the_masked_pair_solve_with_an_all_ones_mask_is_the_plain_one(coupling):
    import psf_est_ref as pr
    s, b = pr.gpu_pair((40, 52), 5)
    ones = np.ones((40, 52) if coupling == "vector" else (40, 52, 3), bool)
    raw, S = er.masked_raw_kernel(b, s, ones, 5, 1e-3, coupling)
    ref, Sr = pr.raw_kernel(b, s, 5, 1e-3, coupling)
    assert np.array_equal(raw, ref) and np.array_equal(S, Sr)
    half = ones.copy()
    half[:, 26:] = False
    raw2, S2 = er.masked_raw_kernel(b, s, half, 5, 1e-3, coupling)
    assert (S2 < S).all() and not np.allclose(raw2, raw)


def test_blind_levels_and_centring():
    assert er.blind_levels(160, 192, 15) == [(3, 40, 48), (7, 80, 96), (15, 160, 192)]
    assert er.blind_levels(80, 104, 5) == [(3, 40, 52), (5, 80, 104)]
    assert er.blind_levels(60, 200, 15) == [(3, 15, 50), (7, 30, 100), (15, 60, 200)] and er.blind_levels(59, 200, 15)[-1][0] != 15
    k = np.zeros((7, 7, 3))
    k[1, 4] = 0.5
    k[2, 5] = 0.5                                                        # centroid (1.5, 4.5) -> rounds to (2, 5): moved by (+1, -2)
    c = er.centred(k)
    assert c[2, 2, 0] == 0.5 and c[3, 3, 0] == 0.5 and abs(c[..., 1].sum() - 1) < 1e-12
    edge = np.zeros((5, 5, 3))
    edge[0, 0] = 0.25
    edge[4, 4] = 0.75                                                    # centroid (3, 3): moved by (-1, -1), the tap at (0, 0) leaves and is dropped
    c = er.centred(edge)
    assert c[3, 3, 0] == 1.0 and c[..., 0].sum() == 1.0


@pytest.mark.parametrize("name", list(er.blind_kernels()))
def test_the_alternation_meets_the_quality_conditions(name):
    """the defaults (edges_ref.BLIND: 5 iterations per level, 4 shock steps of dt 0.4, flat 0.01, keep 2, balance 0.01) on the five cases,
    dead leaves with noise of sigma 0.002, distances allowing a shift of +-2 px; the line of 11 is reported, not gated"""
    sharp, blurred, k, est = er.blind_reference(name)
    K = k.shape[0]
    assert est.shape == (K, K, 3) and np.abs(est.sum(axis=(0, 1)) - 1).max() < 1e-9 and (est >= 0).all()
    q = er.quality(name, est)
    print("blind_psf %s: L1 to truth %.3f, guesses %s, own flip %.3f; rms %.4f -> %.4f (true PSF %.4f)" % (
        name, q["l1"], {n: round(v, 3) for n, v in q["guesses"].items()}, q["flip"], q["rms_blurred"], q["rms_wiener"], er.quality(name, k)["rms_wiener"]))
    er.assert_quality(name, q)
    if name in er.BLIND_GPU_CASES:
        scatter = float(np.abs(est[..., 0] - er.blind_psf(blurred, K, solve_dtype=np.float32)[..., 0]).sum())
        print("  float64 against float32 solve: L1 %.6f (recorded %.6f)" % (scatter, er.BLIND_SCATTER[name]))
        assert scatter <= 1.5 * er.BLIND_SCATTER[name] + 1e-5              # the recorded constants still describe the specification
    if name in ("box5", "box9", "gauss15"):
        assert 0.5 * min(q["guesses"].values()) - q["l1"] >= 10 * er.BLIND_GATE   # the gate is below a tenth of the margin
