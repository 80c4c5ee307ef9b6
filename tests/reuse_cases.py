"""Run kinds, shapes and data for the job-reuse tests (no device needed to build or to route them).

An ics_rl job is kept alive and called again with other pictures, other parameters and other routes (lib/deconvolution.py _get_job,
deblur_module, bench.py's shards, lib/banded.py).  It carries state from call to call, most of it built lazily by the route that first needs
it; STATE names every piece (csrc/ics_host.h ics_rl).  A run KIND is a set of debug switches and run parameters that reaches one route; every
kind says which pieces of STATE its route reads or writes (`owns`) and which kernel families `_native.describe` must report for it (`route`),
so that a kind that silently routes elsewhere fails tests/test_reuse_cases.py instead of testing nothing.
tests/test_gpu_job_reuse.py runs the kinds in sequences on one job and holds the job's state against that of a fresh job, bit for bit.

Three shape families, the smallest on which these routes still differ from one another:
  S1  230 x 260, 15 x 15   3 x 3 mode-2 tiles with rim and far-edge units, 4 x 5 tiles of 64 px, 8 x 9 tiles of 32 px (the small-frame kernel's)
  S2  150 x 140, 51 x 51   two tap blocks a side on the matrix cores: the chain starts from the negated image (blk_negf)
  S3  150 x 140, 87 x 87   tap blocks on the tiles and on the matrix cores, the run-time-sized vector kernels
  S4  230 x 430, 15 x 15   3 x 5 mode-2 tiles.  A mode-2 unit is a pair of row-major neighbours and reads the image's spectra (fspec) only where
                           neither tile touches the frame's rim: S1's 3 x 3 tiles have no such pair (its centre tile travels with a rim tile), so
                           on S1 a stale fspec goes unseen -- a build whose image_changed() left fspec_valid alone passed every test on S1.  Five
                           tile columns are the fewest with one (mode2_pairs)
"""
import dataclasses

import numpy as np

import route_cases as rc

# csrc/ics_common.h IcsDebug: every switch a kind may set, at its default -- route_cases.SWITCH_DEFAULTS and the four it does not carry
SWITCH_DEFAULTS = dict(rc.SWITCH_DEFAULTS, fft_maxg=1, fft_psf1=1, conv_rs=0, key_trace=0)
FLAG_NO_FUSED_GRADK = rc.FLAG_NO_FUSED_GRADK
STEP = 1e-3
SHAPES = {"S1": (230, 260, 15), "S2": (150, 140, 51), "S3": (150, 140, 87), "S4": (230, 430, 15)}
ROWS = (37, 55)          # image rows 37 ... 91: what the row channels of P2 replace (first row, count)

# what a job carries from one call to the next (csrc/ics_host.h, ics_job.hip, ics_run.hip)
STATE = {
    "a": "facc[0], facc[1] + facc_valid[]: accumulator-order image copies, 32- and 64-row tiles",
    "b": "blk_negf + negf_valid: negated image of an even tap-block count",
    "c": "planar mirrors (twins), plf_valid",
    "d": "fspec + fspec_valid: image spectra of mode 2",
    "e": "spec_conv / spec_corr, fft_on",
    "f": "wconv / wcorr / bt_conv / bt_corr (a blind tile run with psf1 leaves them as its first pack_weights built them)",
    "g": "blk_conv / blk_corr tap-block tables",
    "h": "small_part, small_keys, small_bar, small_gen, small_bak, psf_bak",
    "i": "mgs, mgs_wave, mgs_ready, mgs_set",
    "j": "tvf and its mirror",
    "k": "u / ut / u2 rotation, once per outer iteration",
    "l": "psf / psf_next swap, once per inner iteration",
    "m": "u / u2 swap of fuse = 1",
    "n": "e / e2 ping-pong, par, both reduction sets, dofkeys, flags, scal",
}

# include/ics_hip.h ics_rl_route families
MATRIX, BLOCKS, PACKED, SIZED, TILES, SMALL = 1, 2, 3, 4, 5, 6
GK_FUSED_MATRIX, GK_MATRIX, GK_SPLIT, GK_FP32, GK_SIZED, GK_TILES, GK_FUSED_TILES, GK_SMALL = 1, 2, 3, 4, 5, 6, 7, 8


@dataclasses.dataclass(frozen=True)
class Kind:
    id: str
    shape: str
    blind: bool
    conv: int = 0
    tv_mode: int = 0
    fuse: int = 0
    flags: int = 0
    correlation: int = 0
    switches: tuple = ()      # ((name, value), ...) beyond SWITCH_DEFAULTS; `overlap` among them
    owns: str = "kn"          # letters of STATE
    route: tuple = ()         # (conv_family, gradk_family, image_in_accumulator_order) a run of two outer iterations must report

    @property
    def lambd(self):
        return 50.0 if self.tv_mode >= 2 else 10000.0

    def switch(self, name):
        return dict(SWITCH_DEFAULTS, **dict(self.switches))[name]

    def with_(self, **kw):
        """the same kind with other parameters; `overlap=` and the like replace or add a switch"""
        sw = dict(self.switches)
        for k in [k for k in kw if k in SWITCH_DEFAULTS]:
            sw[k] = kw.pop(k)
        return dataclasses.replace(self, switches=tuple(sorted(sw.items())), **kw)


def _k(id, shape, blind, owns, route, **kw):
    sw = tuple(sorted(kw.pop("switches", {}).items()))
    return Kind(id, shape, blind, switches=sw, owns="".join(sorted(set(owns + "kn"))), route=route, **kw)


KINDS = (
    # ---- S1 ------------------------------------------------------------------------------------------------------------------------------
    _k("small", "S1", True, "h", (SMALL, GK_SMALL, 0)),
    _k("small-ov2", "S1", True, "h", (SMALL, GK_SMALL, 0), switches={"overlap": 2}),
    _k("small-ov0", "S1", True, "h", (SMALL, GK_SMALL, 0), switches={"overlap": 0}),
    _k("mx-fused", "S1", True, "af", (MATRIX, GK_FUSED_MATRIX, 1), conv=2),
    _k("mx-nofused", "S1", True, "f", (MATRIX, GK_MATRIX, 0), conv=2, flags=FLAG_NO_FUSED_GRADK),
    _k("mx-nb", "S1", False, "f", (MATRIX, 0, 0), conv=2),
    _k("mx-planar0", "S1", True, "f", (MATRIX, GK_FUSED_MATRIX, 0), conv=2, switches={"planar_image": 0}),
    _k("mx-rs", "S1", True, "af", (MATRIX, GK_FUSED_MATRIX, 1), conv=2, switches={"conv_rs": 2, "fused_rs": 4}),      # 32-row residual tiles + 64-row fused unit: both facc slots
    _k("mx-nb-rs", "S1", False, "af", (MATRIX, 0, 1), conv=2, switches={"conv_rs": 2}),
    _k("mx-fuse1", "S1", True, "fm", (MATRIX, GK_MATRIX, 0), conv=2, fuse=1),
    _k("mx-nb-ov0", "S1", False, "f", (MATRIX, 0, 0), conv=2, switches={"overlap": 0}),
    _k("mx-ov2", "S1", True, "afh", (MATRIX, GK_FUSED_MATRIX, 1), conv=2, switches={"overlap": 2}),                     # (h: psf_bak)
    _k("vec-bl", "S1", True, "f", (PACKED, GK_FP32, 0), conv=1),
    _k("vec-nb-fuse1", "S1", False, "fm", (PACKED, 0, 0), conv=1, fuse=1),
    _k("ti-bl", "S1", True, "cdefl", (TILES, GK_FUSED_TILES, 0), conv=3, switches={"fft_maxg": 0}),
    _k("ti-nb", "S1", False, "cde", (TILES, 0, 0), conv=3),
    _k("ti-bl-maxg2", "S1", True, "cdefil", (TILES, GK_FUSED_TILES, 0), conv=3, switches={"fft_maxg": 2}),
    _k("ti-nb-maxg2", "S1", False, "cdei", (TILES, 0, 0), conv=3, switches={"fft_maxg": 2}),
    _k("ti-bl-two", "S1", True, "ce", (TILES, GK_TILES, 0), conv=3, switches={"fft_conv2": 0, "fft_fused": 0, "fft_psf1": 0}),
    _k("ti-bl-gk0", "S1", True, "cde", (TILES, GK_MATRIX, 0), conv=3, switches={"fft_gradk": 0}),
    _k("ti-bl-corr", "S1", True, "cdefl", (TILES, GK_FUSED_TILES, 0), conv=3, correlation=1),
    _k("tv1-mx", "S1", True, "fj", (MATRIX, GK_FUSED_MATRIX, 0), conv=2, tv_mode=1),
    _k("tv2-ti", "S1", True, "cdej", (TILES, GK_FUSED_TILES, 0), conv=3, tv_mode=2),
    _k("tv3-mx-nb", "S1", False, "fj", (MATRIX, 0, 0), conv=2, tv_mode=3),
    # ---- S2: two tap blocks a side ---------------------------------------------------------------------------------------------------------
    _k("blk-bl", "S2", True, "bg", (BLOCKS, GK_SPLIT, 0)),
    _k("blk-nb", "S2", False, "bg", (BLOCKS, 0, 0)),
    _k("vec51-bl", "S2", True, "f", (PACKED, GK_FP32, 0), conv=1),
    _k("ti51-bl", "S2", True, "cefl", (TILES, GK_FUSED_TILES, 0), conv=3),
    _k("ti51-nb", "S2", False, "ce", (TILES, 0, 0), conv=3),
    _k("tv1-51", "S2", True, "fj", (PACKED, GK_SPLIT, 0), tv_mode=1),
    # ---- S3 --------------------------------------------------------------------------------------------------------------------------------
    _k("ti87-bl", "S3", True, "ce", (TILES, GK_TILES, 0), conv=3),
    _k("blk87-bl", "S3", True, "g", (BLOCKS, GK_SPLIT, 0), conv=2),
    _k("vec87-bl", "S3", True, "", (SIZED, GK_SIZED, 0), conv=1),
    # ---- S4: mode-2 units that read the image's spectra ----------------------------------------------------------------------------------------
    _k("ti4-bl", "S4", True, "cdefl", (TILES, GK_FUSED_TILES, 0), conv=3, switches={"fft_maxg": 0}),
    _k("ti4-nb", "S4", False, "cde", (TILES, 0, 0), conv=3),
    _k("ti4-bl-maxg2", "S4", True, "cdefil", (TILES, GK_FUSED_TILES, 0), conv=3, switches={"fft_maxg": 2}),
    _k("mx4-fused", "S4", True, "af", (MATRIX, GK_FUSED_MATRIX, 1), conv=2),
    _k("tv1-mx4", "S4", True, "fj", (MATRIX, GK_FUSED_MATRIX, 0), conv=2, tv_mode=1),
)
BY_ID = {k.id: k for k in KINDS}
assert len(BY_ID) == len(KINDS)
# the three Bs every kind of S1 runs in front of with 1, 2 and 3 outer iterations; the As that also run under the two further conditions of P1
FIXED_B = ("small", "mx-fused", "ti-bl")
SPECIAL_A = ("small", "mx-fused", "ti-bl", "ti-bl-maxg2")
# the kinds that keep a copy derived from the image (P2), and the kind whose run steps the image on the device, per shape
IMAGE_COPY = ("mx-fused", "mx-rs", "blk-bl", "ti-bl-two", "ti-bl", "ti-bl-maxg2", "ti4-bl", "ti4-bl-maxg2")
IMAGE_STEPPER = {"S1": "tv1-mx", "S2": "tv1-51", "S4": "tv1-mx4"}
# stages on a used job (P3), and reads after a run (P4: one kind per convolution family)
STAGE_A = ("ti-bl", "small", "mx-fused", "tv1-mx")
READ_KINDS = ("mx-fused", "blk-bl", "vec-bl", "vec87-bl", "ti-bl", "small")


def kinds(shape):
    return [k for k in KINDS if k.shape == shape]


def window(shape):
    import rl_mm_oracle as orc
    return orc.default_window(*SHAPES[shape])


def params_of(nv, k, iterations):
    return nv.RLJob.params(*window(k.shape), 1e9, iterations, STEP, k.lambd, k.blind, k.correlation, 3, stop_test=2, fuse=k.fuse, tv_mode=k.tv_mode,
                           conv=k.conv, flags=k.flags)


class switches_set:
    """context manager: the kind's debug switches on (and key_trace), every switch of SWITCH_DEFAULTS back where it was afterwards"""

    def __init__(self, k, key_trace=1):
        self.k, self.key_trace = k, key_trace

    def __enter__(self):
        from lib import _native as nv
        want = dict(SWITCH_DEFAULTS, key_trace=self.key_trace, **dict(self.k.switches))
        self.old = {name: nv.debug_set(name, want[name]) for name in SWITCH_DEFAULTS}
        return self

    def __exit__(self, *exc):
        from lib import _native as nv
        for name, v in self.old.items():
            nv.debug_set(name, v)


def switch_values():
    """{name: current value} of every switch of SWITCH_DEFAULTS"""
    import ctypes as C
    from lib import _native as nv
    out = {}
    for name in SWITCH_DEFAULTS:
        v = C.c_int(0)
        assert nv.load().ics_debug_get(name.encode(), C.byref(v)) == 0, name
        out[name] = v.value
    return out


def describe(k, iterations=2):
    """(conv_family, gradk_family, image_in_accumulator_order) ics_describe gives for a run of this kind"""
    from lib import _native as nv
    with switches_set(k, key_trace=0):
        r = nv.describe(*SHAPES[k.shape], params_of(nv, k, iterations))
    return (r.conv_family, r.gradk_family, r.image_in_accumulator_order)


def mode2_pairs(shape):
    """[True where the pair touches the frame's rim] for the tile pairs of mode 2 on a shape (csrc/ics_conv_fft.hip ics_fft_tile_grid, csrc/ics_fft_tile.h
    decode_unit, tile_rows, tile_is_border): tiles of V = 128 - 2 K + 2 pixels over the u-frame, the last of an axis extended over the pad ring
    where that saves a tile; pairs of row-major neighbours; a pair whose tiles both lie inside the image by a pad reads the image's spectra"""
    M, N, K = SHAPES[shape]
    pad, V = K // 2, rc.FFT_P - 2 * K + 2

    def axis(n):       # [(origin, length stored)] of the tiles along an axis of n image pixels
        un = n + 2 * pad
        cnt = min(-(-un // V), -(-n // V))
        return [(i * V, V if i < cnt - 1 else un - i * V) for i in range(cnt)]

    ys, xs = axis(M), axis(N)
    border = [oy - pad < pad or oy + ry + pad > pad + M or ox - pad < pad or ox + cx + pad > pad + N for oy, ry in ys for ox, cx in xs]
    return [border[i] or (i + 1 < len(border) and border[i + 1]) for i in range(0, len(border), 2)]


def a_iterations(shape, ia, ib):
    """outer iterations of run A in the pair (kind number ia, kind number ib) of a shape: 1, 2, 3 cycling over the pairs"""
    return (ia * len(kinds(shape)) + ib) % 3 + 1


_DATA = {}


def data(shape):
    """{"a": D_a, "b": D_b} of a shape, each a dict(image, u, psf_blind, psf_true): route_cases.make_data's recipe with two seeds, D_b scaled by
    0.7 so that no stale maximum or scale happens to fit, and four different PSFs.  Computed once, never written to."""
    if shape not in _DATA:
        import rl_mm_oracle as orc
        M, N, MK = SHAPES[shape]
        out = {}
        for name, seed, scale in (("a", 1201, 1.0), ("b", 1202, 0.7)):
            image, u0, psf_true = rc.make_data(rc.Case("reuse-" + name, M, N, MK, False, seed=seed + 7 * MK))
            image, u0 = image * np.float32(scale), u0 * np.float32(scale)
            if name == "a":      # a narrower true PSF, and a blind start that is not the uniform one
                psf_true = orc.gaussian_psf(MK, MK / 8.0)
                psf_blind = orc.gaussian_psf(MK, MK / 2.5)
            else:
                psf_blind = orc.uniform_psf(MK)
            d = {"image": np.ascontiguousarray(image, np.float32), "u": np.ascontiguousarray(u0, np.float32),
                 "psf_blind": np.ascontiguousarray(psf_blind, np.float32), "psf_true": np.ascontiguousarray(psf_true, np.float32)}
            for a in d.values():
                a.setflags(write=False)
            out[name] = d
        _DATA[shape] = out
    return _DATA[shape]


def psf_of(d, k):
    return d["psf_blind"] if k.blind else d["psf_true"]
