"""The PSF gradient of a blind run (A12 + A13, lib/deconvolution.pyx:567-571) as the oracle computes it, for the tests that hold the
device's last gradient -- what ics_rl_run leaves in BUF_GRADK -- against float64 (tests/test_gpu_psf_gradient.py), and the wrong gradients
those tests have to tell from the right one (tests/test_psf_gradient_ref.py).  numpy and the oracle only: no device code.

Why the gradient has a gate of its own: the PSF step is normalised, dtpsf = step_factor / MK max psf / max |gradk| (pyx:574), so one inner
iteration moves the PSF by at most step_factor / MK of its maximum whatever the gradient is -- 6.7e-5 at 15 x 15, below the 1e-4 of
max |ref| every whole-run test gates u and the PSF with.

  reference   the oracle's float64 form: conv = "direct" (float64 direct sums), conv = "fft64" (the same sums through float64 FFTs; within
              1e-12 of them) where the direct sums cost more than DIRECT_CAP products a convolution;
  D           the distance of the oracle's own float32 form (conv = "scipy": float32 arrays, complex64 FFTs, the reference's method) from
              that reference, max norm over max |reference|.  Neither involves the code under test;
  gate        FACTOR * D = 8 D: the device differs from both forms (fp32 FMAs in tile order, a slightly different u trajectory over the
              inner iterations) and D samples rounding in one direction only;
  restatement where a device result falls between 8 D and the mutants and the cause is rounding (psf_scale_term: one ulp of the PSF's
              scale), the case's gate is 4 x the distance of a float32 direct-sum run of the oracle from the reference (restatement_f32);
  mutants     the gradients a wrong kernel would give (MUTANTS); every one must lie at least FLOOR = 10 gates from the reference.
"""
import functools
import warnings

import numpy as np

import rl_mm_oracle as orc

STEP, LAMBD = 1e-3, 1e4
FACTOR = 8.0           # gate = FACTOR * D
FLOOR = 10.0           # every mutant at least FLOOR gates away
DIRECT_CAP = 1.2e7     # M N MK^2 up to which the float64 form is the direct sums (255 x 255 / 15 is 1.5e7: float64 FFTs)
TILE = 32              # csrc/ics_small.hip: a workgroup of the small-frame kernel owns a TILE x TILE tile of the u-frame
LANES = 64             # ... and one wave sums the tiles' shares: lane = tile, a second tile per lane from here on


def asymmetric_psf(MK, rng):
    """a Gaussian times 0.5 + random per tap and channel, normalised: no symmetry, so that flips, transposes and swapped channels show"""
    psf = (orc.gaussian_psf(MK) * (0.5 + rng.random((MK, MK, 3), dtype=np.float32))).astype(np.float32)
    orc.normalize_kernel(psf, MK)
    return psf


class Case:
    """image, u0, psf0 of a blind problem (read-only arrays); hashed by (M, N, MK, seed)"""

    def __init__(self, M, N, MK, seed, image, u0, psf0):
        self.M, self.N, self.MK, self.seed, self.pad = M, N, MK, seed, MK // 2
        self.image, self.u0, self.psf0 = image, u0, psf0
        self.key = (M, N, MK, seed)

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, Case) and self.key == other.key

    def __repr__(self):
        return "%dx%d/%d seed %d" % self.key


@functools.lru_cache(maxsize=None)
def case(M, N, MK, seed=0):
    c = orc.synth_case(M, N, MK, seed=seed, blind=True, per_channel_psf=True)
    psf0 = asymmetric_psf(MK, np.random.default_rng(1000003 * seed + M + 7 * N + 31 * MK))
    for a in (c["image"], c["u0"], psf0):
        a.setflags(write=False)
    return Case(M, N, MK, seed, c["image"], c["u0"], psf0)


def small_window(c):
    """a statistics window of a few pixels: it enters nothing before the end of the outer iteration (pyx:593-638), so the gradient does
    not depend on it, and the oracle's float64 autocorrelation of the window costs its area squared"""
    return (1, min(9, c.M), 1, min(9, c.N)) if min(c.M, c.N) >= 4 else (0, c.M, 0, c.N)


def float64_form(c):
    return "direct" if c.M * c.N * c.MK ** 2 <= DIRECT_CAP else "fft64"


def _conv_f32(a, b, mode, reverse=False):
    """orc._conv_direct's sums with float32 products and float32 accumulation, the taps in row-major order or in the reverse of it"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if mode == "valid" and b.shape[0] > a.shape[0]:
        a, b = b, a
    (Ma, Na), (Mb, Nb) = a.shape, b.shape
    taps = [(p, q) for p in range(Mb) for q in range(Nb)]
    if reverse:
        taps.reverse()
    if mode == "valid":
        out = np.zeros((Ma - Mb + 1, Na - Nb + 1), np.float32)
        if Mb * Nb <= out.size:
            for p, q in taps:
                out += b[p, q] * a[Mb - 1 - p:Mb - 1 - p + out.shape[0], Nb - 1 - q:Nb - 1 - q + out.shape[1]]
        else:  # few outputs, long sums (A13): numpy's pairwise float32 sum
            br = b[::-1, ::-1]
            for i in range(out.shape[0]):
                for j in range(out.shape[1]):
                    out[i, j] = np.sum(a[i:i + Mb, j:j + Nb] * br, dtype=np.float32)
        return out
    full = np.zeros((Ma + Mb - 1, Na + Nb - 1), np.float32)
    for p, q in taps:
        full[p:p + Ma, q:q + Na] += b[p, q] * a
    if mode == "same":
        oy, ox = (Mb - 1) // 2, (Nb - 1) // 2
        return full[oy:oy + Ma, ox:ox + Na]
    return full


# forms beyond the oracle's own: float32 direct sums in two tap orders (restatement_f32)
FORMS = {"f32": _conv_f32, "f32-reversed": functools.partial(_conv_f32, reverse=True)}


@functools.lru_cache(maxsize=None)
def _run(c, win, form, correlation, iterations):
    u, psf = c.u0.copy(), c.psf0.copy()
    tr = orc.Trace()
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (varu of a window narrower than 2 pad: an empty slice, pyx:600)
        orc.richardson_lucy_MM(c.image.copy(), u, psf, *win, 1e9, c.M, c.N, 3, c.MK, iterations, STEP, LAMBD, blind=True,
                               correlation=bool(correlation), conv=FORMS.get(form, form), trace=tr, quiet=True)
    assert tr.iterations == iterations and len(tr.gradk) == orc.INNER_ITER * iterations
    for a in tr.gradk + [u]:
        a.setflags(write=False)
    return tr, u


def last_gradient(c, win=None, form="float64", correlation=0, iterations=1):
    """(gradient, dtpsf) of the last inner iteration of `iterations` outer ones of the oracle with conv = form ("float64": the direct sums,
    float64 FFTs above DIRECT_CAP), at step_factor 1e-3 and lambd 1e4"""
    tr = _run(c, win or small_window(c), float64_form(c) if form == "float64" else form, int(correlation), iterations)[0]
    return tr.gradk[-1], tr.dtpsf[-1]


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def D(c, win=None, correlation=0, iterations=1):
    return rel(last_gradient(c, win, "scipy", correlation, iterations)[0], last_gradient(c, win, "float64", correlation, iterations)[0])


def gate(c, win=None, correlation=0, iterations=1):
    return FACTOR * D(c, win, correlation, iterations)


def restatement_f32(c, win=None, correlation=0, iterations=1):
    """the distance of the oracle with float32 direct sums from the float64 form, the larger of two tap orders.  A case whose D happens to
    be small (no ulp flip in the complex64 run, see psf_scale_term) while a float32 evaluation of the same sums does flip is gated by
    F32_FACTOR times this instead of 8 D; the GPU module names those cases."""
    ref = last_gradient(c, win, "float64", correlation, iterations)[0]
    return max(rel(last_gradient(c, win, form, correlation, iterations)[0], ref) for form in FORMS)


F32_FACTOR = 4.0


def psf_scale_term(c, win=None, correlation=0, iterations=1):
    """What one ulp of the PSF's scale does to the gradient.  A16 divides the stepped PSF by its sequential float32 sum (pyx:58-64); two
    correct float32 evaluations of the iteration can land one ulp apart in that divisor.  Every tap of the channel then differs by
    2^-23 of itself, the synthesis by 2^-23 of itself -- 2^-23 image, a constant sign over the frame -- and the gradient adds that up
    coherently:  2^-23 max |A13(u, image)| / max |gradk|.  Rounding elsewhere is incoherent and 50 times smaller (3e-6): the errors of
    float32 direct sums are one or the other, never in between."""
    g = last_gradient(c, win, "float64", correlation, iterations)[0]
    u, _ = inputs(c, win, correlation, iterations)
    return float(2.0 ** -23 * np.abs(gradient_of(c, u, c.image)).max() / np.abs(g).max())


# ---- the inputs of the last gradient, and the mutants --------------------------------------------------------------------------------
def gradient_of(c, u, e):
    """A12 + A13 as the oracle's float64 form evaluates them, rounded to float32 as its gradk array does"""
    cv = {"direct": orc._conv_direct, "fft64": orc._conv_fft64}[float64_form(c)]
    u_rot = orc.rotate_180(u)
    return np.stack([cv(u_rot[..., ch], e[..., ch], "valid") for ch in range(3)], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(c, win=None, correlation=0, iterations=1):
    """(u, residual) that the float64 form's last gradient was computed from.  u is the run's result (nothing writes it after A10 of the
    last inner iteration); the residual is A11 with the PSF before its last step, replayed from psf0 with the recorded gradients and
    step sizes (pyx:574-589, the oracle's own float32 statements).  Checked: A13 of the two gives the recorded gradient bit for bit."""
    form = float64_form(c)
    tr, u = _run(c, win or small_window(c), form, int(correlation), iterations)
    cv = {"direct": orc._conv_direct, "fft64": orc._conv_fft64}[form]
    psf = c.psf0.copy()
    for gk, dtpsf in zip(tr.gradk[:-1], tr.dtpsf[:-1]):
        psf -= dtpsf * gk
        if correlation:
            m = np.mean(psf, axis=2)
            psf = np.dstack((m, m, m))
        orc.normalize_kernel(psf, c.MK)
    e = np.zeros((c.M, c.N, 3), np.float32)
    for ch in range(3):
        e[..., ch] = cv(u[..., ch], psf[..., ch], "valid")
    e -= c.image
    assert np.array_equal(gradient_of(c, u, e), tr.gradk[-1]), c
    e.setflags(write=False)
    return u, e


def tiles(c):
    """(tile rows, tile columns) of the u-frame"""
    return -(-(c.M + 2 * c.pad) // TILE), -(-(c.N + 2 * c.pad) // TILE)


def _without(c, g, u, e, mask):
    """the gradient without the residual pixels of `mask` (image coordinates): their share never reached the sum"""
    if not mask.any():
        return None
    return (g.astype(np.float64) - gradient_of(c, u, np.where(mask[..., None], e, np.float32(0)))).astype(np.float32)


def _uframe_coords(c):
    y, x = np.mgrid[0:c.M, 0:c.N]
    return y + c.pad, x + c.pad          # residual pixel (y, x) sits at (y + pad, x + pad) of the u-frame


def _tile_missing(c, g, u, e):
    ty, tx = tiles(c)
    fy, fx = _uframe_coords(c)
    return _without(c, g, u, e, (fy // TILE == ty // 2) & (fx // TILE == tx // 2))


def _seam_column_missing(c, g, u, e):
    fy, fx = _uframe_coords(c)
    col = TILE if c.N + c.pad > TILE else (c.N + 2 * c.pad) // 2      # the first column of the second tile; one tile across: the middle
    return _without(c, g, u, e, fx == col)


def _tiles_past_64_missing(c, g, u, e):
    ty, tx = tiles(c)
    fy, fx = _uframe_coords(c)
    return _without(c, g, u, e, (fy // TILE) * tx + fx // TILE >= LANES)


def _zeroed(sl):
    def f(c, g, u, e):
        out = g.copy()
        out[sl] = 0
        return out
    return f


# name -> f(case, float64-form gradient, u, residual) -> the wrong gradient, or None where the mutant does not apply to the case
MUTANTS = {
    "transposed": lambda c, g, u, e: np.ascontiguousarray(g.transpose(1, 0, 2)),
    "rotated 180": lambda c, g, u, e: np.ascontiguousarray(g[::-1, ::-1]),
    "shifted one tap down": lambda c, g, u, e: np.roll(g, 1, axis=0),
    "shifted one tap right": lambda c, g, u, e: np.roll(g, 1, axis=1),
    "last tap row zero": _zeroed((slice(-1, None), slice(None))),
    "last tap column zero": _zeroed((slice(None), slice(-1, None))),
    "a tile's share missing": _tile_missing,
    "a residual column at a tile seam missing": _seam_column_missing,
    "tiles past 64 missing": _tiles_past_64_missing,
    "channels 0 and 1 swapped": lambda c, g, u, e: np.ascontiguousarray(g[..., [1, 0, 2]]),
    "channels 1 and 2 swapped": lambda c, g, u, e: np.ascontiguousarray(g[..., [0, 2, 1]]),
}


def separations(c, win=None, correlation=0, iterations=1):
    """{mutant: its max-norm distance from the float64 form's gradient over max |gradient|} for the mutants that apply to the case"""
    g = last_gradient(c, win, "float64", correlation, iterations)[0]
    u, e = inputs(c, win, correlation, iterations)
    out = {}
    for name, f in MUTANTS.items():
        m = f(c, g, u, e)
        if m is not None:
            out[name] = rel(m, g)
    return out
