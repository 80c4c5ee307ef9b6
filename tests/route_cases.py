"""Whole-call cases keyed by the kernel route they run on (no device needed to build the list or to route it).

resolve_route (csrc/ics_route.hip) picks, per run, the convolution family, the PSF-gradient family, the fp16 split and the accumulator-order
image copy; tests/golden/route_table.json names every route it can return.  This module builds a seeded, deterministic list of whole
richardson_lucy_MM calls, each with the debug switches it sets, and records the route `lib._native.describe` returns for it.
tests/test_route_coverage.py checks that every route of the table has a case; tests/test_gpu_route_matrix.py runs every case against the
oracle.  Shapes are drawn where kernels go wrong: tile and unit seams of the transform tiles (128 x 128 overlap-save), 64-px tile seams of
the matrix-core and HWC kernels, the PSF sizes where the compiled kernels change, the largest frames the small-frame kernel takes (and the
first it refuses), degenerate frames.  Forced families keep frames small; one ICS_CONV_AUTO case per family sits near its threshold.
"""
import dataclasses
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_table.json")

# csrc/ics_common.h IcsDebug: the routing / scheduling switches a case may set, at their defaults
SWITCH_DEFAULTS = {"conv_path": 0, "small_iter": 1, "fused_gradk": 1, "fft_gradk": 1, "fft_fused": 1, "fft_conv2": 1, "fft_rot": 1,
                   "planar_image": 1, "fused_rs": 0, "max_wgs": 0, "overlap": 1}
VARIANTS = ("plain", "black_top", "black_left", "black_bottom", "scaled", "flat")     # scripts/dbg/fuzz_runs.py's data variants
FFT_P = 128            # transform tile edge (csrc/ics_conv_fft.hip ICS_FFT_P)
CONV2_MAX_K = 25       # csrc/ics_route.hip ICS_CONV2_MAX_K: A1 + A3 as one unit up to this PSF size
FFT_MAX_K = 85         # csrc/ics_conv_fft.hip ICS_FFT_MAX_K: one tile per PSF up to here, tap blocks above
TILE = 64              # csrc/ics_common.h ICS_TILE
FLAG_NO_FUSED_GRADK = 1
DIRECT_CAP = 4e8       # M N MK^2 up to which the float64 direct-sum oracle is affordable in numpy
# Case ids the GPU matrix does not compare with the oracle.  They do not count as coverage (tests/test_route_coverage.py): a route whose only
# cases are listed here fails the coverage check.
EXCLUDED = frozenset()


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    M: int
    N: int
    MK: int
    blind: bool
    correlation: int = 0
    conv: int = 0
    tv_mode: int = 0
    fuse: int = 0
    flags: int = 0
    switches: tuple = ()          # ((name, value), ...) beyond SWITCH_DEFAULTS
    win: tuple = None             # stats window (top, bottom, left, right) in image coordinates
    variant: tuple = ("plain",)   # (name, parameter)
    iters: int = 2
    seed: int = 0

    @property
    def lambd(self):
        return 50.0 if self.tv_mode >= 2 else 10000.0

    def switch(self, name):
        return dict(SWITCH_DEFAULTS, **dict(self.switches))[name]


def legend():
    """{route tuple: legend character} of tests/golden/route_table.json (error codes left out)"""
    with open(GOLDEN) as fh:
        t = json.load(fh)
    return {tuple(v): k for k, v in t["legend"].items() if isinstance(v, list)}


def table_routes():
    """{tv_mode: set of legend characters} reachable per tv_mode in tests/golden/route_table.json"""
    from test_route_table import PARAMS as params     # the order the table was recorded in
    with open(GOLDEN) as fh:
        t = json.load(fh)
    assert t["params"].startswith("blind, conv, tv_mode, fuse"), t["params"]
    out = {m: set() for m in range(4)}
    for rows in t["table"].values():
        for s in rows.values():
            for q, c in zip(params, s):
                if isinstance(t["legend"][c], list):
                    out[q[2]].add(c)
    return out


def params_of(nv, c):
    return nv.RLJob.params(*c.win, 1e9, c.iters, 1e-3, c.lambd, c.blind, c.correlation, 3, stop_test=1, fuse=c.fuse, tv_mode=c.tv_mode,
                           conv=c.conv, flags=c.flags)


class switches_set:
    """context manager: the case's debug switches on, every routing switch back at its default afterwards"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        from lib import _native as nv
        self.old = {k: nv.debug_set(k, self.c.switch(k)) for k in SWITCH_DEFAULTS}
        return self

    def __exit__(self, *exc):
        from lib import _native as nv
        for k, v in self.old.items():
            nv.debug_set(k, v)


def route_tuple(r):
    from lib import _native as nv
    return tuple(getattr(r, f) for f, _ in nv.RLRoute._fields_[1:])


def describe(c):
    """the route tuple ics_describe gives for this case (with its switches set)"""
    from lib import _native as nv
    with switches_set(c):
        return route_tuple(nv.describe(c.M, c.N, c.MK, params_of(nv, c)))


# ---- edge-biased shapes -------------------------------------------------------------------------------------------------------------------
def tile_valid(MK, conv2):
    """valid output pixels per transform tile along an axis (rows): one convolution 128 - MK + 1, mode 2 (two in a row) 128 - 2 MK + 2"""
    return FFT_P - 2 * MK + 2 if conv2 else FFT_P - MK + 1


def small_limit(MK, blind):
    """largest square side ICS_CONV_AUTO runs on the small-frame kernel (family 6) for this PSF size; the next side is refused"""
    from lib import _native as nv
    p = nv.RLJob.params(1, 2, 1, 2, 1e9, 2, 1e-3, 1e4, blind)
    with switches_set(Case("probe", 8, 8, MK, blind, win=(1, 2, 1, 2))):
        s = 8
        while nv.describe(s + 1, s + 1, MK, p).conv_family == 6:
            s += 1
    return s


def _window(rng, M, N, MK):
    if min(M, N) < 10:
        return (0, M, 0, N)
    top = int(rng.integers(0, M // 3)); left = int(rng.integers(0, N // 3))
    return (top, int(rng.integers(top + 8, M + 1)), left, int(rng.integers(left + 8, N + 1)))


def _build():
    rng = np.random.default_rng(20261016)
    out = []

    def add(tag, M, N, MK, blind, variant=("plain",), **kw):
        seed = int(rng.integers(0, 1 << 30))
        win = kw.pop("win", None) or _window(rng, M, N, MK)
        sw = tuple(sorted(kw.pop("switches", {}).items()))
        cid = "%s-%dx%d-k%d-%s" % (tag, M, N, MK, "bl" if blind else "nb")
        for k, v in sorted(kw.items()):
            cid += "-%s%d" % (k, v)
        for k, v in sw:
            cid += "-%s=%d" % (k, v)
        if variant[0] != "plain":
            cid += "-" + variant[0] + ("%g" % variant[1] if len(variant) > 1 else "")
        out.append(Case(cid, M, N, MK, blind, win=win, switches=sw, variant=variant, seed=seed, **kw))

    # -- transform tiles (conv = 3): tile seams k V + {-1, 0, +1} for one convolution (mode 0/1 tiles) and for mode 2
    for MK, blind in ((15, True), (15, False), (9, True), (25, False), (27, True), (31, False)):
        V = tile_valid(MK, MK <= CONV2_MAX_K)
        for k, d in ((1, -1), (1, 0), (2, 1), (2, -1)):
            s = k * V + d - (2 * (MK // 2) if MK <= CONV2_MAX_K else 0)   # (mode 2's tiles cover the u-frame: its side is M + 2 pad)
            if s >= 4:
                add("fft-seam", s, s + 2 * d + 1 if s + 2 * d + 1 > 4 else s, MK, blind, conv=3)
    V = tile_valid(15, True)
    add("fft-one-tile", V - 20, V - 30, 15, True, conv=3)
    add("fft-one-row", 40, 3 * V + 1, 15, True, conv=3)                 # one tile row, several tile columns
    add("fft-one-col", 3 * V + 1, 40, 15, False, conv=3)                # one tile column, several tile rows (round-5 decode bug)
    add("fft-one-col", 2 * tile_valid(41, False) + 3, 30, 41, True, conv=3)
    for MK in (85, 87):                                                  # one tile / tap blocks on the tiles
        add("fft-blk", 150, 140, MK, True, conv=3)
        add("fft-blk", 140, 150, MK, False, conv=3)
    add("fft-blk", 60, 70, 129, False, conv=3)
    add("fft-blk", 70, 60, 129, True, conv=3)
    for MK in (25, 27):                                                  # both sides of the mode-2 limit
        add("fft-conv2", 2 * tile_valid(MK, MK <= CONV2_MAX_K) + 1, 180, MK, False, conv=3)
    add("fft-conv2", 230, 120, 15, True, conv=3, switches={"fft_conv2": 0})
    add("fft-conv2", 160, 170, 31, False, conv=3, switches={"fft_conv2": 2})
    add("fft-conv2", 140, 150, 27, True, conv=3, switches={"fft_conv2": 2})
    add("fft-rot", 250, 230, 15, False, conv=3, switches={"fft_rot": 0})
    add("fft-wgs", 250, 230, 15, True, conv=3, switches={"max_wgs": 5})
    add("fft-wgs", 200, 210, 41, False, conv=3, switches={"max_wgs": 3})
    add("fft-gk", 150, 160, 21, True, conv=3, switches={"fft_gradk": 0})          # PSF gradient on the matrix cores beside the tiles
    add("fft-gk", 130, 140, 37, True, conv=3, switches={"fft_gradk": 0})          # ... as 31 x 31 tap blocks
    add("fft-nofused", 150, 160, 21, True, conv=3, switches={"fft_fused": 0})
    add("fft-nofused", 150, 130, 13, True, conv=3, flags=FLAG_NO_FUSED_GRADK)
    add("fft-corr", 140, 150, 15, True, conv=3, correlation=1)
    add("fft-corr", 100, 120, 45, True, conv=3, correlation=1)
    # -- matrix cores and HWC kernels: 64 k +- 1 sides, PSF sizes across the compiled-size boundaries
    for MK, blind in ((31, True), (33, True), (37, False), (39, True), (49, False), (51, True), (63, False), (65, True), (127, False), (129, True)):
        for conv in (2, 1):
            if conv == 2 and MK > 49 and MK not in (51, 65, 129):
                continue
            if conv == 1 and MK > 127:
                continue
            k = 1 + int(rng.integers(1, 3))
            add("hwc", TILE * k + 1, TILE * (k - 1) - 1 + MK // 2, MK, blind, conv=conv if not (conv == 2 and MK > 49) else 0)
    for MK, blind in ((3, True), (7, False), (13, True), (15, True), (17, False), (17, True), (21, True), (23, False), (25, True)):
        add("mfma", TILE * 3 - 1, TILE * 2 + 1, MK, blind, conv=2)
        add("fp32", TILE * 2 + 1, TILE * 3 - 1, MK, blind, conv=1)
    add("mfma-fused-rs", 200, 190, 9, True, conv=2, switches={"fused_rs": 2})
    add("mfma-fused-rs", 190, 200, 13, True, conv=2, switches={"fused_rs": 4})
    add("mfma-nofused", 130, 190, 9, True, conv=2, flags=FLAG_NO_FUSED_GRADK)
    add("mfma-nofused", 130, 150, 11, True, conv=2, switches={"fused_gradk": 0})
    add("mfma-planar", 190, 130, 11, True, conv=2, switches={"planar_image": 0})
    add("mfma-planar", 150, 170, 19, False, conv=2, switches={"planar_image": 0})
    add("mfma-planar", 170, 150, 19, True, conv=2, switches={"planar_image": 0})
    add("mfma-wgs", 257, 193, 9, True, conv=2, switches={"max_wgs": 7})
    add("mfma-overlap", 129, 191, 7, False, conv=2, switches={"overlap": 2})
    add("path", 150, 140, 11, True, switches={"conv_path": 2, "small_iter": 0})
    add("path", 140, 150, 21, False, switches={"conv_path": 1})
    for conv, MK in ((1, 9), (2, 15), (3, 21), (1, 71), (0, 55)):           # correlation on every conv family
        add("corr", 130, 120, MK, True, conv=conv, correlation=1)
    # -- fuse = 1: the update fused into the next convolution (u ping-pong)
    add("fuse", 150, 170, 9, True, conv=2, fuse=1)
    add("fuse", 130, 150, 21, False, conv=2, fuse=1)
    add("fuse", 140, 130, 13, True, conv=1, fuse=1)
    add("fuse", 130, 131, 31, False, conv=1, fuse=1)
    # -- small-frame kernel: 32 k +- 1 sides up to the largest frame it takes, and the first it refuses
    for MK, blind in ((3, True), (15, True), (31, True), (23, False)):
        lim = small_limit(MK, blind)
        for s in sorted({32 * 2 + 1, 32 * 4 - 1, 32 * (lim // 32) - 1, lim, lim + 1}):
            if s <= lim + 1 and s >= MK:
                add("small", s, s if s != lim else lim - 32 + 1, MK, blind)
    add("small", 255, 255, 15, True, switches={"small_iter": 2})
    add("small", 97, 129, 9, True, correlation=1)
    # -- degenerate frames: narrower than the PSF, one row, one column
    add("degen", 5, 40, 9, False, conv=1)
    add("degen", 40, 5, 9, True, conv=2)
    add("degen", 7, 30, 11, True)
    add("degen", 1, 9, 3, False)
    add("degen", 65, 1, 3, True)
    add("degen", 1, 70, 5, True, conv=2)
    add("degen", 60, 1, 5, False, conv=1)
    add("degen", 6, 50, 15, False, conv=3)
    add("degen", 50, 3, 7, True, conv=3)
    # -- ICS_CONV_AUTO near each family's threshold (the automatic choice itself)
    add("auto", 680, 670, 51, False)        # tiles from 0.5 Mpx at 51 ... 85 (u-frame 730 x 720)
    add("auto", 630, 620, 51, False)        # just below: tap blocks on the matrix cores
    add("auto", 600, 610, 51, True)
    add("blk", 150, 140, 67, False, conv=2)
    add("auto", 1000, 1010, 21, True)       # tiles from 1 Mpx blind at 19 ... 49
    add("auto", 420, 400, 33, True)         # matrix cores, gradient as tap blocks
    add("auto", 380, 330, 15, False)        # matrix cores (small frames stop at ~290 px here)
    add("auto", 300, 290, 7, True)          # first frames past the small-frame kernel
    add("auto", 200, 220, 71, True)         # tap blocks on the matrix cores
    # -- the PAM kinds and the active MM-TV kind (tv_mode 1 ... 3) on every family that takes them
    for tv in (1, 2, 3):
        for conv, MK, blind in ((0, 9, True), (0, 19, True), (0, 37, True), (0, 55, True), (1, 9, True), (1, 33, True), (2, 13, True),
                                (2, 19, False), (2, 25, True), (2, 41, True), (3, 15, False), (3, 21, True), (3, 45, True)):
            if tv == 1 and conv == 3:
                continue
            add("tv%d" % tv, 100 + MK, 110 + MK // 2, MK, blind, conv=conv, tv_mode=tv)
        add("tv%d" % tv, 120, 130, 13, True, conv=2, tv_mode=tv, switches={"planar_image": 0})
        if tv >= 2:
            add("tv%d" % tv, 140, 150, 21, True, conv=3, tv_mode=tv, switches={"fft_gradk": 0})
            add("tv%d" % tv, 140, 150, 37, True, conv=3, tv_mode=tv, switches={"fft_gradk": 0})
            add("tv%d" % tv, 150, 140, 21, True, conv=3, tv_mode=tv, switches={"fft_fused": 0})
            add("tv%d" % tv, 170, 180, 19, True, conv=2, tv_mode=tv)
    for tv in (1, 2, 3):
        add("tv%d" % tv, 90, 100, 7, False, conv=1, tv_mode=tv)
        add("tv%d" % tv, 100, 90, 25, False, conv=2, tv_mode=tv)
    # -- data variants (scripts/dbg/fuzz_runs.py) on several families
    for i, (MK, conv, blind) in enumerate(((9, 2, True), (15, 3, True), (21, 1, False), (7, 0, True), (13, 3, False), (33, 2, True))):
        M, N = 90 + 17 * i, 110 + 13 * i
        add("var", M, N, MK, blind, ("black_top", int(rng.integers(1, M // 2))), conv=conv)
        add("var", M, N, MK, blind, ("black_left", int(rng.integers(1, N // 2))), conv=conv)
        add("var", M, N, MK, blind, ("black_bottom", int(rng.integers(1, M // 2))), conv=conv)
        add("var", M, N, MK, blind, ("scaled", float(10.0 ** int(rng.integers(-6, 5)))), conv=conv)
        add("var", M, N, MK, blind, ("flat",), conv=conv)
    add("var", 120, 110, 15, True, ("scaled", 1e-6), conv=3)
    add("var", 110, 120, 15, False, ("scaled", 1e4), conv=2)
    return out


_CASES = None
_ROUTES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
        ids = [c.id for c in _CASES]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return _CASES


def routes():
    """{case id: legend character of the route describe() gives} (recorded once per process)"""
    global _ROUTES
    if _ROUTES is None:
        leg = legend()
        _ROUTES = {}
        for c in cases():
            t = describe(c)
            assert t in leg, (c.id, t)
            _ROUTES[c.id] = leg[t]
    return _ROUTES


def make_data(c):
    """(image, u0, psf0) of a case: a smoothed random scene blurred by a Gaussian PSF (float64 FFT convolution) plus 1e-3 noise, u0 = the
    image edge-padded (deconvolve.py:303), psf0 = uniform (blind) or the true PSF; then the case's data variant."""
    from scipy.signal import fftconvolve
    import rl_mm_oracle as orc
    rng = np.random.default_rng(c.seed)
    M, N, MK = c.M, c.N, c.MK
    pad = MK // 2
    sharp = orc._smooth7(rng.random((M + 2 * pad, N + 2 * pad, 3), dtype=np.float32).astype(np.float64)) * 0.8 + 0.1
    psf_true = orc.gaussian_psf(MK).astype(np.float64)
    image = np.stack([fftconvolve(sharp[..., k], psf_true[..., k], mode="valid") for k in range(3)], axis=-1)
    image = np.ascontiguousarray(image + 1e-3 * rng.standard_normal(image.shape), dtype=np.float32)
    u0 = np.ascontiguousarray(np.pad(image, ((pad, pad), (pad, pad), (0, 0)), mode="edge"), dtype=np.float32)
    psf0 = orc.uniform_psf(MK) if c.blind else np.ascontiguousarray(psf_true, dtype=np.float32)
    v = c.variant
    if v[0] == "black_top":
        image[:v[1]] = 0; u0[:v[1] + pad] = 0
    elif v[0] == "black_left":
        image[:, :v[1]] = 0; u0[:, :v[1] + pad] = 0
    elif v[0] == "black_bottom":
        image[-v[1]:] = 0; u0[-(v[1] + pad):] = 0
    elif v[0] == "scaled":
        image *= np.float32(v[1]); u0 *= np.float32(v[1])
    elif v[0] == "flat":
        image[:] = np.float32(0.37); u0[:] = np.float32(0.37)
    return image, u0, np.ascontiguousarray(psf0, dtype=np.float32)


def route_map():
    """{legend character: [case ids]} over the cases the GPU matrix compares with the oracle"""
    out = {}
    for cid, r in routes().items():
        if cid not in EXCLUDED:
            out.setdefault(r, []).append(cid)
    return out


def cheapest_per_route():
    """{(tv_mode, legend character): the cheapest case of that route and tv_mode by M N MK^2 iters} over the cases the GPU matrix compares
    with the oracle: one whole call per route for checks that repeat a call several times (tests/test_gpu_pool_check.py)"""
    R = routes()
    out = {}
    for c in cases():
        if c.id in EXCLUDED:
            continue
        key = (c.tv_mode, R[c.id])
        cost = c.M * c.N * c.MK ** 2 * c.iters
        if key not in out or cost < out[key][0]:
            out[key] = (cost, c)
    return {k: v[1] for k, v in out.items()}


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "image-cases-studies_amd"), os.path.join(root, "oracle")):
        sys.path.insert(0, p)
    leg = {v: k for k, v in legend().items()}
    for r, ids in sorted(route_map().items()):
        print(r, list(leg[r]), len(ids), ids[:4])
