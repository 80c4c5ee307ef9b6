"""The stop-test statistics of one window (csrc/ics_stats.hip: M_r, Hu, varu; lib/deconvolution.pyx:600-601, 627-638) in numpy, without the
project's library: a float64 reference, a float32 restatement in the order the device takes, residual fields on which M_r depends on
where each lag is read, and named mutants of the reference, one indexing mistake each.

Why these fields: on a noise-like residual M_r is the zero-lag peak and little else, so reading the autocorrelation one lag row or
column off moves it by 1e-4 .. 1e-6, below any gate a float32 transform can meet (tests/test_stats_ref.py asserts this once).  A field
that is almost zero except for a pair of impulses has an autocorrelation of three peaks per channel: the zero lag and the pair's
separation, both signs.  With the separations at the extreme lags that are read, one lag off loses or gains a whole peak."""
import functools

import numpy as np

import rl_mm_oracle as orc

F32 = np.float32
GENERATORS = ("pairs", "pairs_outside", "comb", "rough")
MR_CAP, HU_CAP = 2e-4, 1e-5     # the gates of tests/test_gpu_stages.py::test_window_statistics_and_whiteness_metric: no gate here is above them
GATE_FACTOR = 4                 # what the device may order differently from the restatement (as tests/test_gpu_guided.py)


# ---- the transform sizes of a window, as ensure_window (csrc/ics_job.hip) picks them --------------------------------------------
def transform_sizes(H, W):
    """(P, 0, 0) on the P x P path, (0, Py, Px) on the long-line path"""
    P = 2
    while P < 2 * max(H, W) - 1:
        P <<= 1
    if P <= 8192:
        return P, 0, 0
    Py = Px = 64
    while Py < 2 * H - 1:
        Py <<= 1
    while Px < 2 * W - 1:
        Px <<= 1
    return 0, Py, Px


def lines_per_workgroup(L):
    """C of k_fft_cols / k_big_cols for in-LDS lines of L points"""
    return 1 if L < 4 else (4 if L <= 1024 else (2 if L <= 2048 else 1))


# ---- residual fields (seeded, float32, never written) ---------------------------------------------------------------------------
def _floor(H, W, rng):
    return (rng.random((H, W, 3)) * 1e-3).astype(F32)


def _put_pair(f, k, dy, dx, rng):
    H, W = f.shape[:2]
    dy, dx = min(dy, H - 1), max(min(dx, W - 1), 1 - W)  # below 3 px: whatever separation exists
    y0, x0 = int(rng.integers(0, H - dy)), int(rng.integers(max(0, -dx), W - max(0, dx)))
    f[y0, x0, k] = 1.0
    f[y0 + dy, x0 + dx, k] = 1.0


def pairs(H, W, seed):
    """one pair of unit impulses per channel, separated by the extreme lags that are read: (H//2, W//2) -- the corner lag row -(H//2),
    lag column -(W//2) --, (H-1-H//2, 0) and (0, W-1-W//2); the zero lag row and column come with the last two"""
    rng = np.random.default_rng([seed, H, W, 1])
    f = _floor(H, W, rng)
    for k, (dy, dx) in enumerate(((H // 2, W // 2), (H - 1 - H // 2, 0), (0, W - 1 - W // 2))):
        _put_pair(f, k, dy, dx, rng)
    return f


def pairs_outside(H, W, seed):
    """separations that are not read with either sign: H//2 + 1 rows, W//2 + 1 columns, and the anti-diagonal (H - H//2, -(W - W//2)),
    whose two peaks lie past the last lag row on one side and past the last lag column on the other (an even side reads one lag more
    on the negative side than on the positive one: a field with a peak at lag column +W/2 alone needs a row that is not read either)"""
    rng = np.random.default_rng([seed, H, W, 2])
    f = _floor(H, W, rng)
    for k, (dy, dx) in enumerate(((H // 2 + 1, 0), (0, W // 2 + 1), (H - H // 2, -(W - W // 2)))):
        _put_pair(f, k, dy, dx, rng)
    return f


def comb(H, W, seed):
    """8 to 16 impulses of unequal height per channel: many distinct lags carry weight at once"""
    rng = np.random.default_rng([seed, H, W, 3])
    f = _floor(H, W, rng)
    for k in range(3):
        n = min(int(rng.integers(8, 17)), H * W)
        at = rng.choice(H * W, size=n, replace=False)
        f[at // W, at % W, k] = rng.uniform(0.3, 1.0, n).astype(F32)
    return f


def rough(H, W, seed):
    """a noise frame minus a 3 x 3 box blur of another: what ICS_STAGE_SYNTH_RESIDUAL leaves of a random u and image (the field of
    tests/test_gpu_stages.py and tests/test_gpu_big_windows.py)"""
    rng = np.random.default_rng([seed, H, W, 4])
    u = rng.random((H + 2, W + 2, 3))
    blur = sum(u[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    return (rng.random((H, W, 3)) - blur).astype(F32)


def field(gen, H, W, seed):
    f = {"pairs": pairs, "pairs_outside": pairs_outside, "comb": comb, "rough": rough}[gen](H, W, seed)
    f.setflags(write=False)
    return f


# ---- float64 reference ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def weights64(H, W):
    w = orc.stop_weights(0, H, 0, W).astype(np.float64)
    w.setflags(write=False)
    return w


def _fast_len(n):
    try:
        from scipy.fft import next_fast_len
        return next_fast_len(n, real=True)
    except ImportError:
        return 1 << (n - 1).bit_length()


def autocorrelation64(e_win):
    """(A, fy, fx): A[k][dy % fy, dx % fx] = sum_pq t[p, q, k] t[p - dy, q - dx, k] of the normalised window, transform lengths past
    2 H + 2, 2 W + 2 so that no lag within one step of the window's size wraps around"""
    e = np.asarray(e_win, np.float64)
    H, W = e.shape[:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (e - e.mean()) / e.std()
        t = t / np.max(np.abs(t))
    fy, fx = _fast_len(2 * H + 3), _fast_len(2 * W + 3)
    A = []
    for k in range(3):
        F = np.fft.rfft2(t[..., k], s=(fy, fx))
        A.append(np.fft.irfft2(F.real ** 2 + F.imag ** 2, s=(fy, fx)))
    return A, fy, fx


def m_r64(e_win, A=None, *, drow=0, dcol=0, wrapped_rows=0, past_cols=0, n0=None, transposed_weights=False, scale=1.0, planes=(0, 1, 2)):
    """M_r = mean(ac^2 w), ac[r, b] = autocorrelation at lag (r - H//2, b - W//2), written with the device's index maps (lag row l of
    k_fft_mr: l < n0 is lag l and weight row l + H//2, l >= n0 lag l - H and weight row l - n0) so that each keyword is one slip"""
    H, W = e_win.shape[:2]
    A, fy, fx = A or autocorrelation64(e_win)
    n0 = H - H // 2 if n0 is None else n0
    l = np.arange(H)
    lag_y = np.where(l < n0, l, l - H) + drow + wrapped_rows * (l >= n0)
    wrow = np.where(l < n0, l + H // 2, l - n0)
    b = np.arange(W)
    lag_x = b - W // 2 + dcol + past_cols * (b > W // 2)
    w = weights64(H, W)
    w = w.ravel()[b[None, :] * H + wrow[:, None]] if transposed_weights else w[wrow]
    s = 0.0
    for k in planes:
        ac = A[k][np.ix_(lag_y % fy, lag_x % fx)] * scale
        s += np.sum(ac * ac * w)
    return s / (3.0 * H * W)


def reference(e_win, u_win):
    """(M_r, Hu, varu) in float64, pyx:600-601 and 627-638; NaN where numpy gives NaN (a 1 x 1 window, an empty u window)"""
    e = np.asarray(e_win, np.float64)
    H, W = e.shape[:2]
    u = np.asarray(u_win, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        varu = float(np.var(u)) if u.size else float("nan")
        return float(m_r64(e_win)), float(np.sum(e * e) / (3.0 * H * W)), varu


# ---- mutants of the reference: one named mistake each ---------------------------------------------------------------------------
def _long_line_scale(H, W):
    P, Py, Px = transform_sizes(H, W)
    return 1.0 if P else float(Py) * Px / float(max(Py, Px)) ** 2      # 1 / max(Py, Px)^2 in place of 1 / (Py Px)


MUTANTS = {
    "lag row +1": lambda e, A: m_r64(e, A, drow=1),
    "lag row -1": lambda e, A: m_r64(e, A, drow=-1),
    "lag column +1": lambda e, A: m_r64(e, A, dcol=1),
    "rows l >= n0 one up": lambda e, A: m_r64(e, A, wrapped_rows=1),
    "rows l >= n0 one down": lambda e, A: m_r64(e, A, wrapped_rows=-1),
    "columns past W//2 one up": lambda e, A: m_r64(e, A, past_cols=1),
    "columns past W//2 one down": lambda e, A: m_r64(e, A, past_cols=-1),
    "n0 = H//2": lambda e, A: m_r64(e, A, n0=e.shape[0] // 2),
    "weights [b * H + r]": lambda e, A: m_r64(e, A, transposed_weights=True),
    "long-line scale of the larger axis": lambda e, A: m_r64(e, A, scale=_long_line_scale(*e.shape[:2])),
    "one plane twice": lambda e, A: m_r64(e, A, planes=(0, 0, 2)),
}


def exact_symmetry(name, H, W):
    """why mutant `name` cannot change M_r on an H x W window (None where it can).  Two facts: ac(dy, dx) = ac(-dy, -dx), and the
    weights are mirror-symmetric in rows and in columns."""
    if name == "lag row +1" and H % 2 == 0 and W % 2 == 1:
        return "even H reads lag rows -H/2 .. H/2-1; one up is the mirror image -(H/2-1) .. H/2, and with odd W the columns mirror too"
    if name == "lag column +1" and W % 2 == 0 and H % 2 == 1:
        return "even W reads lag columns -W/2 .. W/2-1; one up is their mirror image, and with odd H the rows mirror too"
    if name == "n0 = H//2" and H % 2 == 0:
        return "H//2 = H - H//2 for even H: the same code"
    if name == "weights [b * H + r]" and (H == W or H == 1 or W == 1):
        return "the weights of a square window are a symmetric matrix; with one row or column b * H + r is r * W + b"
    if name == "long-line scale of the larger axis" and transform_sizes(H, W)[0]:
        return "the P x P path has one transform size"
    if name.startswith("rows l >= n0") and H == 1:
        return "one row: n0 = 1 and no lag row wraps"
    if name.startswith("columns past W//2") and W <= 2:
        return "no column lies past W//2"
    return None


# ---- float32 restatement, in the device's order ---------------------------------------------------------------------------------
def _table(P):
    """ensure_window's twiddles: each entry from its own angle in double, stored as float"""
    ang = -2.0 * np.pi * np.arange(P, dtype=np.float64) / float(P)
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def _stockham(xr, xi, tw, inverse, ts):
    """fft_lines: radix-2 Stockham autosort over the last axis, float32, real and imaginary parts apart so that every product and
    sum rounds once (the library is built without contraction); unscaled; ts = stride into a table of a ts times longer line"""
    L = xr.shape[-1]
    t, p, lead = L // 2, 1, xr.shape[:-1]
    while p < L:
        k = np.arange(p) * (t // p) * ts
        wr, wi = tw[0][k], (-tw[1][k] if inverse else tw[1][k])
        u0r, u0i = xr[..., :t].reshape(lead + (t // p, p)), xi[..., :t].reshape(lead + (t // p, p))
        vr, vi = xr[..., t:].reshape(lead + (t // p, p)), xi[..., t:].reshape(lead + (t // p, p))
        u1r, u1i = vr * wr - vi * wi, vr * wi + vi * wr
        yr, yi = np.empty(lead + (t // p, 2, p), F32), np.empty(lead + (t // p, 2, p), F32)
        yr[..., 0, :] = u0r + u1r; yr[..., 1, :] = u0r - u1r
        yi[..., 0, :] = u0i + u1i; yi[..., 1, :] = u0i - u1i
        xr, xi = yr.reshape(lead + (L,)), yi.reshape(lead + (L,))
        p <<= 1
    return xr, xi


def _chunks(n, L):
    step = max(1, (1 << 22) // L)
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def autocorrelation32(z, Py, Px):
    """z: (3, H, W) float32, the normalised window.  Returns acc (3, H, W) float32, lag row l in the device's order (l < n0: lag l,
    else lag l - H), column b at lag b - W//2, before the scale 1 / (Py Px): k_big_rows, k_big_cols, k_big_mr of ics_stats.hip, lines
    above 8192 points split into N2 in-LDS blocks.  With N2 = 1 and Py = Px = P these are k_fft_rows, k_fft_cols, k_fft_mr: the extra
    factor is W^0 = (1, 0), and a product with it is exact."""
    _, H, W = z.shape
    Ly, Lx = min(Py, 8192), min(Px, 8192)
    N2y, N2x = Py // Ly, Px // Lx
    twy, twx = _table(Py), _table(Px)
    n0 = H - H // 2
    # rows: block k2 of the spectrum (kept in this permuted order) = FFT_L of y_k2[n1] = sum_n2 x[n1 + L n2] W^(k2 (n1 + L n2))
    x = np.zeros((3 * H, N2x * Lx), F32)
    x[:, :W] = z.reshape(3 * H, W)
    m = np.arange(N2x * Lx)
    Zr, Zi = np.empty((3 * H, Px), F32), np.empty((3 * H, Px), F32)
    for k2 in range(N2x):
        tr, ti = twx[0][(k2 * m) % Px], twx[1][(k2 * m) % Px]
        vr, vi = np.zeros((3 * H, Lx), F32), np.zeros((3 * H, Lx), F32)
        for n2 in range(N2x):
            s = slice(n2 * Lx, (n2 + 1) * Lx)
            vr, vi = vr + x[:, s] * tr[s], vi + x[:, s] * ti[s]
        for a, b in _chunks(3 * H, Lx):
            Zr[a:b, k2 * Lx:(k2 + 1) * Lx], Zi[a:b, k2 * Lx:(k2 + 1) * Lx] = _stockham(vr[a:b], vi[a:b], twx, False, N2x)
    # columns: forward, |Z|^2, inverse, combined over the N2y blocks into the H lag rows that are read
    l = np.arange(H)
    zrow = np.where(l < n0, l, l + (Py - H))
    r_all = np.arange(N2y * Ly)
    Cr, Ci = np.empty((3, H, Px), F32), np.empty((3, H, Px), F32)
    for k in range(3):
        for a, b in _chunks(Px, Ly):
            cr, ci = np.zeros((b - a, N2y * Ly), F32), np.zeros((b - a, N2y * Ly), F32)
            cr[:, :H], ci[:, :H] = Zr[k * H:(k + 1) * H, a:b].T, Zi[k * H:(k + 1) * H, a:b].T
            accr, acci = np.zeros((b - a, H), F32), np.zeros((b - a, H), F32)
            for k2 in range(N2y):
                tr, ti = twy[0][(k2 * r_all) % Py], twy[1][(k2 * r_all) % Py]
                dr, di = cr * tr - ci * ti, cr * ti + ci * tr
                vr, vi = np.zeros((b - a, Ly), F32), np.zeros((b - a, Ly), F32)
                for n2 in range(N2y):
                    s = slice(n2 * Ly, (n2 + 1) * Ly)
                    vr, vi = vr + dr[:, s], vi + di[:, s]
                fr, fi = _stockham(vr, vi, twy, False, N2y)
                qr, qi = _stockham(fr * fr + fi * fi, np.zeros_like(fr), twy, True, N2y)
                tr, ti = twy[0][(k2 * zrow) % Py], twy[1][(k2 * zrow) % Py]
                gr, gi = qr[:, zrow % Ly], qi[:, zrow % Ly]
                accr, acci = accr + (gr * tr + gi * ti), acci + (gi * tr - gr * ti)
            Cr[k, :, a:b], Ci[k, :, a:b] = accr.T, acci.T
    # inverse rows of the lag rows: the N2x inverse blocks combined for the W lags read
    col = (np.arange(W) - W // 2) % Px
    acc = np.zeros((3 * H, W), F32)
    Cr, Ci = Cr.reshape(3 * H, Px), Ci.reshape(3 * H, Px)
    for k2 in range(N2x):
        tr, ti = twx[0][(k2 * col) % Px], twx[1][(k2 * col) % Px]
        for a, b in _chunks(3 * H, Lx):
            qr, qi = _stockham(Cr[a:b, k2 * Lx:(k2 + 1) * Lx], Ci[a:b, k2 * Lx:(k2 + 1) * Lx], twx, True, N2x)
            acc[a:b] = acc[a:b] + (qr[:, col % Lx] * tr + qi[:, col % Lx] * ti)
    return acc.reshape(3, H, W)


def restatement_f32(e_win, u_win):
    """(M_r, Hu, varu) in float32 arithmetic as csrc/ics_stats.hip orders it: sums in double, the mean rounded to float, (e - mean),
    / std, / (max|e - mean| / std), the radix-2 Stockham transforms with ensure_window's table, ac * 1 / (Py Px), (ac * ac) * w, the
    sum of that in double"""
    e = np.ascontiguousarray(e_win, F32)
    H, W = e.shape[:2]
    ne = 3 * H * W
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = F32(np.sum(e, dtype=np.float64) / ne)
        v = e - mean
        std = np.sqrt(F32(np.sum(v.astype(np.float64) ** 2) / ne))
        mx = np.max(np.abs(v)) / std
        z = np.ascontiguousarray(np.moveaxis((v / std) / mx, 2, 0))
        P, Py, Px = transform_sizes(H, W)
        Py, Px = (Py, Px) if Py else (P, P)
        ac = autocorrelation32(z, Py, Px) * (F32(1.0) / (F32(Py) * F32(Px)))
        l = np.arange(H)
        n0 = H - H // 2
        w = orc.stop_weights(0, H, 0, W)[np.where(l < n0, l + H // 2, l - n0)]
        M_r = F32(np.sum(((ac * ac) * w).astype(np.float64)) / ne)
        Hu = F32(np.sum(e.astype(np.float64) ** 2) / (3.0 * H * W))
        u = np.ascontiguousarray(u_win, F32)
        varu = F32("nan")
        if u.size:
            du = u - F32(np.sum(u, dtype=np.float64) / u.size)
            sd = np.sqrt(F32(np.sum(du.astype(np.float64) ** 2) / u.size))
            varu = sd * sd
    assert all(isinstance(q, F32) for q in (M_r, Hu, varu, std, mx)) and z.dtype == ac.dtype == w.dtype == F32
    return float(M_r), float(Hu), float(varu)


# ---- the cases, shared by tests/test_stats_ref.py (CPU) and tests/test_gpu_stats_windows.py ------------------------------------
MK = 3
PAD = MK // 2
TOP, LEFT = 4, 7            # where a window sits in its frame unless the case says otherwise: unequal, and not at the origin
SEED = 20


class Case:
    def __init__(self, klass, H, W, gens, frame=None, at=(TOP, LEFT)):
        self.klass, self.H, self.W, self.gens = klass, H, W, gens
        self.top, self.left = at
        self.M, self.N = frame or (H + TOP + 5, W + LEFT + 5)
        self.win = (self.top, self.top + H, self.left, self.left + W)
        self.sizes = transform_sizes(H, W)
        self.id = "%dx%d%s" % (H, W, "" if at == (TOP, LEFT) and not frame else "@%d,%d" % at)
        assert self.win[1] <= self.M and self.win[3] <= self.N

    def __repr__(self):
        return self.id

    def error_frame(self, gen):
        """the M x N residual: `gen`'s field in the window, rough noise around it"""
        e = np.array(rough(self.M, self.N, SEED + 1))
        e[self.win[0]:self.win[1], self.win[2]:self.win[3]] = field(gen, self.H, self.W, SEED)
        return e

    def u_frame(self):
        return np.random.default_rng([SEED, self.M, self.N]).random((self.M + 2 * PAD, self.N + 2 * PAD, 3), dtype=F32)

    def u_window(self, u):
        """pyx:600 on a window that ends inside the frame"""
        return u[self.top + PAD:self.win[1] - PAD, self.left + PAD:self.win[3] - PAD]


ALL3 = ("pairs", "pairs_outside", "comb")
# class: the transform form a window is there to reach
CASES = [Case("P2", 1, 1, ("comb",)),
         Case("P4-8", 2, 3, ALL3), Case("P4-8", 3, 2, ALL3), Case("P4-8", 2, 2, ALL3), Case("P4-8", 1, 2, ALL3),
         Case("P16-64", 4, 5, ALL3), Case("P16-64", 8, 8, ALL3), Case("P16-64", 15, 16, ALL3), Case("P16-64", 16, 17, ALL3), Case("P16-64", 32, 32, ALL3),
         Case("fit128-P256", 64, 64, ALL3), Case("fit128-P256", 65, 64, ALL3),
         Case("degenerate", 1, 300, ALL3), Case("degenerate", 300, 1, ALL3), Case("degenerate", 2, 511, ALL3),
         Case("P1024", 257, 256, ALL3), Case("P1024", 512, 40, ALL3),
         Case("P2048", 513, 64, ALL3), Case("P2048", 64, 1024, ALL3), Case("P2048", 1024, 1023, ALL3),
         Case("P4096", 1025, 32, ALL3),
         Case("P8192", 2149, 301, ("pairs", "pairs_outside"), frame=(2300, 400), at=(100, 30)),
         Case("corner-P256", 71, 100, ALL3, frame=(91, 120), at=(20, 20)), Case("corner-P256", 71, 100, ALL3, frame=(91, 120), at=(0, 0))]
# P >= 2 max(H, W) - 1: 2 x 3 and 3 x 2 take P = 8; P = 4 (where C goes from 1 to 4) needs a longer side of 2, P = 32 one of 9 .. 16.
# 1 x 1 (P = 2, C = 1) has a deviation, and a finite M_r, only where its three channels differ: `comb` there, and NaN asserted for a grey one.
EXPECTED_P = [2, 8, 8, 4, 4, 16, 16, 32, 64, 64, 128, 256, 1024, 1024, 1024, 1024, 1024, 2048, 2048, 2048, 4096, 8192, 256, 256]
BIG_CASES = [Case("Py64-C4", 20, 4200, ALL3), Case("Py2048-C2", 513, 4200, ALL3), Case("Px32768-N2x4", 30, 8300, ALL3),
             Case("Py16384-even", 4600, 330, ALL3), Case("Py16384-odd", 4601, 331, ALL3)]
EXPECTED_PYX = [(64, 16384), (2048, 16384), (64, 32768), (16384, 1024), (16384, 1024)]
MOMENTS = Case("moments", 700, 701, ("rough",))
MOMENTS_MEAN_E, MOMENTS_MEAN_U = 1000.0, 250.0


def moments_frames():
    """(e, u): a residual and a u with large means, so that (x - mean) cancels five digits"""
    e = (MOMENTS.error_frame("rough") + F32(MOMENTS_MEAN_E)).astype(F32)
    u = (MOMENTS.u_frame() + F32(MOMENTS_MEAN_U)).astype(F32)
    return e, u


def gates(case_id):
    """the gates of M_r, Hu, varu on one case: 4 x the restatement's own error, the worst over the case's fields (one scalar's error on one
    field can lie far below float32 rounding by accident: 1.2e-8 for M_r on one of them), never above the present gates"""
    rows = [v for (cid, _), v in F32_RESTATEMENT_ERROR.items() if cid == case_id]
    worst = [max(r[i] for r in rows) for i in range(3)]          # (an empty u window: NaN in every row, and no gate is applied)
    return (min(GATE_FACTOR * worst[0], MR_CAP), min(GATE_FACTOR * worst[1], HU_CAP), min(GATE_FACTOR * worst[2], HU_CAP))


# |restatement_f32 - reference| / |reference| of (M_r, Hu, varu) per case and field, measured on the CPU by `python tests/test_stats_ref.py`
# without the code under test (NaN: the u window is empty and varu is NaN on both sides)
F32_RESTATEMENT_ERROR = {
    ("1x1", "comb"): (4.403e-08, 5.395e-08, float("nan")),
    ("2x3", "pairs"): (1.618e-07, 5.041e-08, float("nan")),
    ("2x3", "pairs_outside"): (8.182e-08, 3.298e-08, float("nan")),
    ("2x3", "comb"): (1.838e-07, 3.620e-08, float("nan")),
    ("3x2", "pairs"): (2.741e-07, 1.834e-08, float("nan")),
    ("3x2", "pairs_outside"): (1.233e-07, 1.302e-08, float("nan")),
    ("3x2", "comb"): (2.504e-07, 6.293e-09, float("nan")),
    ("2x2", "pairs"): (4.900e-08, 3.381e-08, float("nan")),
    ("2x2", "pairs_outside"): (9.659e-08, 3.707e-08, float("nan")),
    ("2x2", "comb"): (8.789e-08, 8.412e-09, float("nan")),
    ("1x2", "pairs"): (3.419e-08, 3.944e-08, float("nan")),
    ("1x2", "pairs_outside"): (4.829e-08, 4.037e-09, float("nan")),
    ("1x2", "comb"): (5.204e-07, 1.962e-08, float("nan")),
    ("4x5", "pairs"): (1.139e-07, 3.257e-08, 1.372e-07),
    ("4x5", "pairs_outside"): (2.046e-07, 1.078e-08, 1.372e-07),
    ("4x5", "comb"): (1.179e-07, 3.468e-10, 1.372e-07),
    ("8x8", "pairs"): (3.939e-08, 2.595e-08, 2.541e-08),
    ("8x8", "pairs_outside"): (2.148e-07, 1.670e-08, 2.541e-08),
    ("8x8", "comb"): (1.283e-07, 1.324e-08, 2.541e-08),
    ("15x16", "pairs"): (2.299e-07, 1.057e-08, 1.086e-08),
    ("15x16", "pairs_outside"): (1.171e-07, 2.854e-08, 1.086e-08),
    ("15x16", "comb"): (9.396e-08, 2.694e-08, 1.086e-08),
    ("16x17", "pairs"): (1.851e-07, 2.026e-09, 6.715e-08),
    ("16x17", "pairs_outside"): (2.883e-07, 2.423e-08, 6.715e-08),
    ("16x17", "comb"): (3.461e-07, 2.220e-08, 6.715e-08),
    ("32x32", "pairs"): (1.605e-07, 3.807e-08, 4.245e-08),
    ("32x32", "pairs_outside"): (7.241e-08, 4.340e-08, 4.245e-08),
    ("32x32", "comb"): (3.449e-07, 1.333e-08, 4.245e-08),
    ("64x64", "pairs"): (1.216e-07, 2.863e-08, 5.327e-09),
    ("64x64", "pairs_outside"): (1.812e-07, 4.244e-08, 5.327e-09),
    ("64x64", "comb"): (1.680e-07, 1.183e-08, 5.327e-09),
    ("65x64", "pairs"): (2.122e-07, 1.222e-08, 3.704e-08),
    ("65x64", "pairs_outside"): (1.581e-07, 1.495e-08, 3.704e-08),
    ("65x64", "comb"): (2.130e-07, 1.722e-10, 3.704e-08),
    ("1x300", "pairs"): (2.071e-07, 3.210e-08, float("nan")),
    ("1x300", "pairs_outside"): (9.423e-08, 1.674e-08, float("nan")),
    ("1x300", "comb"): (2.565e-07, 2.063e-08, float("nan")),
    ("300x1", "pairs"): (1.091e-07, 1.881e-08, float("nan")),
    ("300x1", "pairs_outside"): (7.692e-08, 1.302e-08, float("nan")),
    ("300x1", "comb"): (2.759e-07, 4.147e-09, float("nan")),
    ("2x511", "pairs"): (2.346e-07, 3.016e-08, float("nan")),
    ("2x511", "pairs_outside"): (7.563e-08, 4.278e-08, float("nan")),
    ("2x511", "comb"): (3.806e-08, 2.573e-08, float("nan")),
    ("257x256", "pairs"): (1.944e-07, 4.808e-08, 3.615e-08),
    ("257x256", "pairs_outside"): (2.650e-07, 4.669e-08, 3.615e-08),
    ("257x256", "comb"): (1.876e-07, 2.213e-08, 3.615e-08),
    ("512x40", "pairs"): (1.471e-07, 1.481e-08, 6.398e-08),
    ("512x40", "pairs_outside"): (1.148e-07, 3.140e-08, 6.398e-08),
    ("512x40", "comb"): (2.359e-07, 2.263e-08, 6.398e-08),
    ("513x64", "pairs"): (1.276e-07, 1.228e-09, 3.272e-08),
    ("513x64", "pairs_outside"): (2.760e-07, 4.363e-08, 3.272e-08),
    ("513x64", "comb"): (9.557e-08, 3.878e-08, 3.272e-08),
    ("64x1024", "pairs"): (1.608e-07, 3.618e-10, 1.189e-07),
    ("64x1024", "pairs_outside"): (2.087e-07, 3.212e-08, 1.189e-07),
    ("64x1024", "comb"): (2.494e-07, 3.537e-08, 1.189e-07),
    ("1024x1023", "pairs"): (4.023e-07, 1.363e-09, 6.883e-08),
    ("1024x1023", "pairs_outside"): (2.187e-07, 2.599e-08, 6.883e-08),
    ("1024x1023", "comb"): (4.349e-07, 9.533e-09, 6.883e-08),
    ("1025x32", "pairs"): (1.570e-07, 5.345e-08, 5.475e-09),
    ("1025x32", "pairs_outside"): (1.987e-07, 4.584e-08, 5.475e-09),
    ("1025x32", "comb"): (1.671e-07, 9.004e-09, 5.475e-09),
    ("2149x301@100,30", "pairs"): (2.318e-07, 2.685e-08, 1.259e-07),
    ("2149x301@100,30", "pairs_outside"): (1.343e-07, 1.308e-09, 1.259e-07),
    ("71x100@20,20", "pairs"): (2.941e-07, 2.247e-08, 2.221e-08),
    ("71x100@20,20", "pairs_outside"): (3.219e-07, 1.403e-08, 2.221e-08),
    ("71x100@20,20", "comb"): (2.612e-07, 1.905e-08, 2.221e-08),
    ("71x100@0,0", "pairs"): (2.941e-07, 2.247e-08, 1.051e-08),
    ("71x100@0,0", "pairs_outside"): (3.219e-07, 1.403e-08, 1.051e-08),
    ("71x100@0,0", "comb"): (2.612e-07, 1.905e-08, 1.051e-08),
    ("20x4200", "pairs"): (2.007e-07, 9.202e-09, 6.872e-08),
    ("20x4200", "pairs_outside"): (1.229e-08, 2.071e-08, 6.872e-08),
    ("20x4200", "comb"): (2.457e-07, 3.092e-08, 6.872e-08),
    ("513x4200", "pairs"): (3.294e-07, 1.194e-08, 1.020e-07),
    ("513x4200", "pairs_outside"): (1.706e-07, 4.463e-08, 1.020e-07),
    ("513x4200", "comb"): (3.392e-07, 1.905e-08, 1.020e-07),
    ("30x8300", "pairs"): (2.346e-07, 3.920e-08, 5.380e-08),
    ("30x8300", "pairs_outside"): (1.270e-07, 3.174e-09, 5.380e-08),
    ("30x8300", "comb"): (1.972e-07, 3.348e-08, 5.380e-08),
    ("4600x330", "pairs"): (2.451e-07, 3.231e-08, 1.313e-07),
    ("4600x330", "pairs_outside"): (3.022e-07, 2.596e-08, 1.313e-07),
    ("4600x330", "comb"): (2.603e-07, 5.407e-08, 1.313e-07),
    ("4601x331", "pairs"): (2.296e-07, 9.229e-09, 1.289e-07),
    ("4601x331", "pairs_outside"): (1.775e-07, 2.245e-08, 1.289e-07),
    ("4601x331", "comb"): (9.862e-08, 3.468e-08, 1.289e-07),
    ("700x701", "rough"): (1.038e-04, 1.412e-08, 1.298e-07),
}
