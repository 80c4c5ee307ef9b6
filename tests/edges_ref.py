"""Edge prediction in numpy, the specification of ics_img_shock / ics_img_edge_mask (DeviceImage.shock, DeviceImage.edge_mask;
csrc/ics_img_edges.hip) with the dtype as a parameter: float64 is the oracle, float32 the restatement the device must equal bit for
bit (every operation below is one correctly rounded numpy operation in the order the kernels use; no FMA; IEEE square roots).

Shock filter, one step.  Every plane exists on the picture only; a neighbour is read with the edge repeated (np.pad(mode="edge") of
that plane, each on its own):
    Y    = ((R + G) + B) * dtype(float32(1 / 3))          "vector"; "channel": Y = the channel itself, three times
    Ys   = V(H(Y)),  H(a)[x] = ((a[x-1] + a[x+1]) + (a[x] + a[x])) * 0.25 along x, V the same along y
    L    = ((Ys[x-1] + Ys[x+1]) + (Ys[y-1] + Ys[y+1])) - 4 Ys
    s    = min(max(L * dtype(1 / float32(flat)), -1), 1)
    a, b = u - u[x-1], u[x+1] - u;  c, d = u - u[y-1], u[y+1] - u          per channel u
    m(p, q) = sign(p) min(|p|, |q|) where p q > 0, else 0
    g    = sqrt(m(a, b)^2 + m(c, d)^2)
    out  = u - (float32(dt) s) g

Gradient selection:
    gx, gy = u[x+1] - u, u[y+1] - u per channel, 0 in the last column / row
    "vector":  g = sqrt((q0 + q1) + q2), q_c = gx_c^2 + gy_c^2;  sx = (gx0 + gx1) + gx2, sy likewise; one plane
    "channel": g = sqrt(q_c), sx = gx_c, sy = gy_c; three planes, each selected on its own
    sector: none where not g > 0; 0 where |sy| <= T |sx|; 2 where |sx| <= T |sy|; else 1 where sx sy > 0, else 3     T = float32(0.41421357)
    t_b  = the per_sector-th largest g of sector b, its smallest where it holds fewer;  t = min of t_b over the sectors that hold any
    mask = g >= t;  kept = mask.sum();  all four sectors empty: ValueError("no gradients to select")

The pair solve under a mask (DeviceImage.psf_raw(mask=), ics_img_psf_estimate_masked): tests/psf_est_ref.py with step 3 changed for the
sharp frame only -- dx[y, x] = w[y, x] (mask[y, x] (s[y, x+1] - s[y, x])), dy likewise, the mask H x W ("vector") or H x W x 3
("channel"), 0 or 1; the energy S is summed over what remains; the blurred frame's derivatives are psf_est_ref's.
"""
import functools

import numpy as np
import scipy.fft as sfft

import psf_est_ref as pr
import wiener_ref as wr

COUPLINGS = ("channel", "vector")
SHOCK = (4, 0.4, 0.01)                # iterations, dt, flat: the defaults of DeviceImage.shock
SHOCK_BLOCK = 4                       # steps per launch of the blocked route (ICS_IMG_SHOCK_BLOCK)
TAN_22_5 = np.float32(0.41421357)
# One shock step, float32 against float64: the gate of tests/test_edges.py and why it holds.  u is of order 1, the step adds dt s g
# with |s| <= 1, g of the order of a difference of two pixels: roundings of 6e-8 relative in u, g and s (s = L / flat amplifies the
# rounding of L, a sum of nine values of order 1, by 1 / flat = 100: about 100 x 4 x 6e-8 = 2.4e-5 where |s| < 1) times dt g <= 0.4.
ONE_STEP_GATE = 1e-4


def _edge(a, axis):
    """a with its first and last entry along `axis` repeated: (a[-1], a[+1]) as views of the padded plane"""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (1, 1)
    p = np.pad(a, pad, mode="edge")
    n = a.shape[axis]
    return np.take(p, range(0, n), axis=axis), np.take(p, range(2, n + 2), axis=axis)


def _b121(a, axis, dtype):
    lo, hi = _edge(a, axis)
    return ((lo + hi) + (a + a)) * dtype(0.25)


def _minmod(p, q, dtype):
    return np.where(p * q > 0, np.sign(p) * np.minimum(np.abs(p), np.abs(q)), dtype(0))


def luma(f, dtype):
    return ((f[..., 0] + f[..., 1]) + f[..., 2]) * dtype(np.float32(1.0 / 3.0))


def steer(f, flat, coupling, dtype=np.float64):
    """s of one step: H x W ("vector") or H x W x 3 ("channel")"""
    f = np.asarray(f, dtype=dtype)
    Y = luma(f, dtype) if coupling == "vector" else f
    Ys = _b121(_b121(Y, 1, dtype), 0, dtype)
    l, r = _edge(Ys, 1)
    u, d = _edge(Ys, 0)
    lap = ((l + r) + (u + d)) - dtype(4) * Ys
    s = np.minimum(np.maximum(lap * dtype(1.0 / float(np.float32(flat))), dtype(-1)), dtype(1))
    assert s.dtype == dtype
    return s


def shock_step(f, dt, flat, coupling, dtype=np.float64):
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    f = np.asarray(f, dtype=dtype)
    s = steer(f, flat, coupling, dtype)
    ds = dtype(np.float32(dt)) * s
    if coupling == "vector":
        ds = ds[..., None]
    l, r = _edge(f, 1)
    u, d = _edge(f, 0)
    mx, my = _minmod(f - l, r - f, dtype), _minmod(f - u, d - f, dtype)
    g = np.sqrt(mx * mx + my * my)
    out = f - ds * g
    assert out.dtype == dtype
    return out


def shock(f, iterations=SHOCK[0], dt=SHOCK[1], flat=SHOCK[2], coupling="vector", dtype=np.float64):
    f = np.asarray(f, dtype=dtype)
    for _ in range(iterations):
        f = shock_step(f, dt, flat, coupling, dtype)
    return f


def gradient_keys(f, coupling, dtype=np.float64):
    """(g, sector): P x H x W each, P = 1 ("vector") or 3 ("channel"); sector 4 = none"""
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    f = np.asarray(f, dtype=dtype)
    gx, gy = np.zeros_like(f), np.zeros_like(f)
    gx[:, :-1] = f[:, 1:] - f[:, :-1]
    gy[:-1] = f[1:] - f[:-1]
    q = gx * gx + gy * gy
    if coupling == "vector":
        g = np.sqrt((q[..., 0] + q[..., 1]) + q[..., 2])[None]
        sx, sy = ((gx[..., 0] + gx[..., 1]) + gx[..., 2])[None], ((gy[..., 0] + gy[..., 1]) + gy[..., 2])[None]
    else:
        g, sx, sy = np.moveaxis(np.sqrt(q), 2, 0), np.moveaxis(gx, 2, 0), np.moveaxis(gy, 2, 0)
    T = dtype(TAN_22_5)
    ax, ay = np.abs(sx), np.abs(sy)
    sector = np.where(ay <= T * ax, 0, np.where(ax <= T * ay, 2, np.where(sx * sy > 0, 1, 3)))
    sector = np.where(g > 0, sector, 4)
    assert g.dtype == dtype
    return g, sector


def select(g, sector, per_sector):
    """(mask, t, kept) of one plane"""
    if per_sector < 1:
        raise ValueError("per_sector %r" % (per_sector,))
    ts = []
    for b in range(4):
        v = g[sector == b]
        if v.size:
            k = v.size - min(per_sector, v.size)             # rank from below of the per_sector-th largest
            ts.append(np.partition(v, k)[k])
    if not ts:
        raise ValueError("no gradients to select")
    t = min(ts)
    mask = g >= t
    return mask, t, int(mask.sum())


def edge_mask(f, per_sector, coupling="vector", dtype=np.float64):
    """(mask, t, kept): "vector" an H x W bool array, a scalar, an int; "channel" H x W x 3, three thresholds, three counts"""
    g, sector = gradient_keys(f, coupling, dtype)
    res = [select(g[p], sector[p], per_sector) for p in range(g.shape[0])]
    if coupling == "vector":
        return res[0]
    return np.stack([r[0] for r in res], axis=2), np.array([r[1] for r in res], dtype), tuple(r[2] for r in res)


def masked_raw_kernel(b, s, mask, K, regularisation=pr.REGULARISATION, coupling="vector", dtype=np.float64):
    """psf_est_ref.raw_kernel with the sharp frame's derivatives under the mask: (raw K x K x 3, energy of 3 entries)"""
    b, s, mask = np.asarray(b), np.asarray(s), np.asarray(mask)
    H, W, _ = s.shape
    assert b.shape == s.shape and K % 2 == 1 and 3 <= K <= min(H, W, 255) and regularisation > 0 and coupling in COUPLINGS
    assert mask.shape == ((H, W) if coupling == "vector" else (H, W, 3))
    m = (mask != 0).astype(dtype)
    m = m[..., None] if m.ndim == 2 else m
    Py, Px = wr.sizes(H, W, K)
    assert max(Py, Px) <= wr.MAX_SIDE
    f = s.astype(dtype)
    w = (pr.taper(H, K, dtype)[:, None] * pr.taper(W, K, dtype)[None, :])[..., None]
    ds = np.zeros((2, Py, Px, 3), dtype)
    ds[0, :H, :W - 1] = w[:, :W - 1] * (m[:, :W - 1] * (f[:, 1:] - f[:, :-1]))
    ds[1, :H - 1, :W] = w[:H - 1] * (m[:H - 1] * (f[1:] - f[:-1]))
    db = pr.derivatives(b, K, Py, Px, dtype)
    A, B = sfft.fft2(ds, axes=(1, 2)), sfft.fft2(db, axes=(1, 2))
    N = (np.conj(A) * B).sum(axis=0)
    D = (A.real * A.real + A.imag * A.imag).sum(axis=0)
    S = (ds * ds).sum(axis=(0, 1, 2))
    if coupling == "vector":
        N, D, S = (np.repeat(v.sum(axis=-1, keepdims=True), 3, axis=-1) for v in (N, D, S))
    full = sfft.ifft2(N / (D + dtype(regularisation) * S), axes=(0, 1)).real
    idx_y, idx_x = (np.arange(K) - K // 2) % Py, (np.arange(K) - K // 2) % Px
    raw = full[idx_y][:, idx_x]
    assert raw.dtype == dtype and raw.shape == (K, K, 3)
    return raw, S.astype(np.float64)


def frame(shape, seed=0):
    """a test picture of the given (H, W): soft-edged discs and bars of every orientation on a gradient, blurred ramps for the shock
    filter to steepen, a little noise; float32 in (0, 1)"""
    H, W = shape
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.empty((H, W, 3))
    for c in range(3):
        a = 0.3 + 0.2 * x / max(W - 1, 1) + 0.1 * c * y / max(H - 1, 1)
        for _ in range(6):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.5, 0.3 * min(H, W) + 2)
            a += rng.uniform(-0.25, 0.25) / (1 + np.exp((np.hypot(y - cy, x - cx) - r) / rng.uniform(0.6, 2.0)))
        for _ in range(4):
            th, off = rng.uniform(0, np.pi), rng.uniform(0, 1)
            a += rng.uniform(-0.15, 0.15) / (1 + np.exp(((y - off * H) * np.cos(th) + (x - off * W) * np.sin(th)) / rng.uniform(0.5, 2.5)))
        f[..., c] = a
    f += rng.normal(0, 0.002, f.shape)
    return np.clip(f, 0.01, 0.99).astype(np.float32)


# ---- the alternation: lib.utils.blind_psf ------------------------------------------------------------------------------------------------
# Levels: K_0 = size, K_{l+1} = max(3, (K_l // 2) | 1) until 3; level l works on the frame resized to ceil(H / 2^l) x ceil(W / 2^l) (the
# resize of DeviceImage.resize: oracle/resize_oracle.py); levels whose smaller side falls below 4 K_l are dropped; coarsest first.  Per
# level the PSF of the coarser one is brought to K_l by the same resize, clipped at 0 and normalised.  Per iteration: latent = frame on the
# first iteration of the coarsest level, wiener(frame, psf, balance) otherwise; p = shock(latent); mask = edge_mask(p, per_sector);
# raw = masked_raw_kernel(frame, p, mask); psf = centred(project(raw, threshold)).  per_sector starts at ceil(keep sqrt(H_l W_l) K_l / 4)
# and grows by 1 / 0.9 per iteration (rounded up where it is used).
BLIND = dict(iterations=5, shock=SHOCK, keep=2.0, regularisation=1e-3, threshold=0.05, balance=0.01)


# The end-to-end gate of tests/test_gpu_blind_psf.py, L1(device PSF, specification PSF) on channel 0.  Measured: the L1 between this
# specification with its Wiener and solve steps in float64 and the same in float32 (solve_dtype), the scatter rounding alone produces
# through the discrete mask --
#   python -c "import sys; sys.path[:0] = ['tests', 'oracle']; import numpy as np, edges_ref as er; [print(n, '%.6f' % np.abs(er.blind_psf(er.blind_case(n)[1], K)[..., 0] - er.blind_psf(er.blind_case(n)[1], K, solve_dtype=np.float32)[..., 0]).sum()) for n, K in (('box5', 5), ('box9', 9), ('ell9', 9))]"
# prints box5 0.000137, box9 0.000313, ell9 0.000402.  The gate is four times the largest (the device's transform sums in another order
# and its resize is float32).  It stays below a tenth of the smallest margin by which a quality condition on an L1 distance holds
# (tests/test_edges.py prints them: Gaussian 15, 0.274 - 0.125 = 0.149).
BLIND_SCATTER = {"box5": 0.000137, "box9": 0.000313, "ell9": 0.000402}
BLIND_GATE = 4 * max(BLIND_SCATTER.values())
BLIND_GPU_CASES = ("box5", "box9", "ell9")


def blind_levels(H, W, size):
    """[(K_l, H_l, W_l)], coarsest first"""
    Ks = [int(size)]
    while Ks[-1] > 3:
        Ks.append(max(3, (Ks[-1] // 2) | 1))
    out = []
    for l, K in enumerate(Ks):
        Hl, Wl = -(-H // 2 ** l), -(-W // 2 ** l)
        if min(Hl, Wl) >= 4 * K:
            out.append((K, Hl, Wl))
    return out[::-1]


def shifted(k, dy, dx):
    """k moved by whole pixels, taps leaving the support dropped"""
    K = k.shape[0]
    out = np.zeros_like(k)
    ys, yd = (slice(0, K - dy), slice(dy, K)) if dy >= 0 else (slice(-dy, K), slice(0, K + dy))
    xs, xd = (slice(0, K - dx), slice(dx, K)) if dx >= 0 else (slice(-dx, K), slice(0, K + dx))
    out[yd, xd] = k[ys, xs]
    return out


def centred(psf):
    """every plane shifted by whole pixels so that its centroid rounds to the centre, then renormalised (float64)"""
    psf = np.asarray(psf, dtype=np.float64)
    K = psf.shape[0]
    r = np.arange(K, dtype=np.float64)
    out = np.empty_like(psf)
    for c in range(3):
        p = psf[..., c]
        cy, cx = float((p.sum(axis=1) * r).sum() / p.sum()), float((p.sum(axis=0) * r).sum() / p.sum())
        q = shifted(p, K // 2 - int(np.floor(cy + 0.5)), K // 2 - int(np.floor(cx + 0.5)))
        out[..., c] = q / q.sum()
    return out


def psf_to_size(psf, K):
    import resize_oracle
    p = np.maximum(resize_oracle.resize_scipy(np.asarray(psf, dtype=np.float64), (K, K)), 0.0)
    return p / p.sum(axis=(0, 1))


def blind_psf(src, size, iterations=BLIND["iterations"], shock_args=BLIND["shock"], keep=BLIND["keep"], regularisation=BLIND["regularisation"],
              threshold=BLIND["threshold"], balance=BLIND["balance"], coupling="vector", solve_dtype=np.float64, info=False):
    """the PSF (size x size x 3 float64) of one blurred H x W x 3 frame.  The shock filter and the mask are evaluated in float32, as on the
    device; solve_dtype is the precision of the Wiener and solve steps (float64: the specification; float32: the scatter rounding alone
    produces through the discrete mask)."""
    import resize_oracle
    src = np.asarray(src, dtype=np.float32)
    H, W, _ = src.shape
    levels = blind_levels(H, W, size)
    if not levels:
        raise ValueError("a %d x %d window is smaller than 4 x size = %d" % (H, W, 4 * size))
    psf, kept, rejected = None, [], []
    for K, Hl, Wl in levels:
        frame_l = src if (Hl, Wl) == (H, W) else resize_oracle.resize_scipy(src, (Hl, Wl)).astype(np.float32)
        if psf is not None:
            psf = psf_to_size(psf, K)
        per_sector = float(np.ceil(keep * np.sqrt(Hl * Wl) * K / 4))
        for _ in range(iterations):
            latent = frame_l if psf is None else wr.wiener(frame_l, psf.astype(np.float32), balance, solve_dtype).astype(np.float32)
            p = shock(latent, *shock_args, coupling, np.float32)
            mask, _, k = edge_mask(p, int(np.ceil(per_sector)), coupling, np.float32)
            raw, _ = masked_raw_kernel(frame_l, p, mask, K, regularisation, coupling, solve_dtype)
            proj, rej = pr.project(raw.astype(np.float32), threshold)
            psf = centred(proj)
            per_sector /= 0.9
        kept.append(k)
        rejected.append(tuple(float(v) for v in rej))
    return (psf, levels, kept, rejected) if info else psf


def l1_shift(est, true, reach=2):
    """the smallest L1 distance of channel 0 of est, moved by up to `reach` pixels either way, to channel 0 of true"""
    e, t = np.asarray(est, np.float64)[..., 0], np.asarray(true, np.float64)[..., 0]
    return min(float(np.abs(shifted(e, dy, dx) - t).sum()) for dy in range(-reach, reach + 1) for dx in range(-reach, reach + 1))


def blind_kernels():
    """name -> (K, H, W, K x K kernel of sum 1): the five cases of the quality conditions"""
    def norm(k):
        return k / k.sum()
    ell = np.zeros((9, 9))
    ell[1:8, 2:5] = 1.0                       # an upright bar three pixels wide ...
    ell[5:8, 2:8] = 1.0                       # ... and a foot to the right: an L whose centroid rounds to the centre
    r = np.arange(15) - 7
    line = np.zeros((11, 11))
    line[5, :] = 1.0
    return {"box5": (5, 80, 104, norm(np.ones((5, 5)))), "box9": (9, 160, 192, norm(np.ones((9, 9)))),
            "gauss15": (15, 160, 192, norm(np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * (15 / 4.0) ** 2)))),
            "ell9": (9, 160, 192, norm(ell)), "line11": (11, 160, 192, norm(line))}


def blind_case(name, sigma=0.002):
    """(sharp, blurred float32, K x K x 3 PSF) on the project's dead leaves"""
    from scipy.ndimage import convolve
    K, H, W, k = blind_kernels()[name]
    rng = np.random.default_rng(4000 + K + H)
    big = wr.dead_leaves(rng, H + 2 * K, W + 2 * K)
    blurred = np.dstack([convolve(big[..., c], k, mode="nearest") for c in range(3)])[K:-K, K:-K]     # (scipy.ndimage.convolve: a true convolution)
    blurred = (blurred + rng.normal(0, sigma, blurred.shape)).astype(np.float32)
    return big[K:-K, K:-K], blurred, np.dstack([k] * 3)


def trivial_guesses(K):
    """the delta, the uniform kernel and the centred Gaussian of wiener_ref.three_psfs, K x K each"""
    delta = np.zeros((K, K))
    delta[K // 2, K // 2] = 1.0
    return {"delta": delta, "uniform": np.ones((K, K)) / K ** 2, "gaussian": wr.three_psfs(K)[..., 1]}


@functools.lru_cache(maxsize=None)
def blind_reference(name):
    """(sharp, blurred, true PSF, the specification's PSF) of a case, computed once: do not write to them"""
    sharp, blurred, k = blind_case(name)
    est = blind_psf(blurred, k.shape[0])
    for a in (sharp, blurred, k, est):
        a.setflags(write=False)
    return sharp, blurred, k, est


def quality(name, est, wiener_of=None):
    """the figures of the quality conditions for an estimate of a case: L1 to the truth, to every trivial guess that is not the truth,
    of the estimate's 180-degree flip, and the rms error to the sharp frame of the blurred frame and of wiener(blurred, est)"""
    sharp, blurred, k, _ = blind_reference(name)
    K = k.shape[0]
    guesses = {n: l1_shift(np.dstack([g] * 3), k) for n, g in trivial_guesses(K).items()}
    guesses = {n: v for n, v in guesses.items() if v > 1e-9}
    rms = lambda a: float(np.sqrt(np.mean((np.asarray(a, np.float64) - sharp) ** 2)))
    restored = (wiener_of or (lambda f, p: wr.wiener(f, p, BLIND["balance"])))(blurred, np.asarray(est, np.float32))
    return {"l1": l1_shift(est, k), "guesses": guesses, "flip": l1_shift(np.asarray(est)[::-1, ::-1], k), "rms_blurred": rms(blurred), "rms_wiener": rms(restored)}


def assert_quality(name, q):
    """the conditions of the issue; line11 is reported only"""
    if name in ("box5", "box9", "gauss15"):
        assert q["l1"] <= 0.5 * min(q["guesses"].values()), (name, q)
    if name == "ell9":
        assert q["l1"] < min(q["guesses"].values()) and q["l1"] < q["flip"], (name, q)
    if name != "line11":
        assert q["rms_wiener"] < q["rms_blurred"], (name, q)
