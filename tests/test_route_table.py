"""The routing table of ics_describe, pinned field by field (CPU only: ics_describe needs no device).

Every kernel family a run launches is decided by one function of csrc/ics_route.hip (resolve_route).  This sweep covers the regimes
that function separates -- the small-frame kernel, the matrix cores, the transform tiles, tap blocks, the run-time-sized kernels and
the edge where the planar mirrors stop fitting 2 GiB (18784 x 9256 / 33) -- over blind / non-blind, params.conv 0-3, tv_mode 0-3, fuse,
ICS_FLAG_NO_FUSED_GRADK and the routing switches, and compares every field of ics_rl_route (or the error code, where describe refuses
the case) with tests/golden/route_table.json.  That table was recorded from the library as it was before the routing was gathered
into resolve_route, by running `sweep` below with `_native.debug_set` and writing `encode(...)` of the result."""
import itertools
import json
import os
import string

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_table.json")

SHAPES = [
    (96, 80, 9), (160, 160, 7), (255, 255, 15), (255, 255, 23), (290, 290, 31), (512, 512, 15),   # small frames (the last: 64-px tiles only)
    (1024, 1024, 7), (1024, 1024, 21), (2048, 2048, 15), (2048, 2048, 45),                  # matrix cores, split gradient
    (4096, 4096, 9), (4096, 4096, 15), (2900, 2900, 17), (2048, 2048, 25), (2048, 2048, 67), (4096, 4096, 97),   # transform tiles
    (1024, 1024, 63), (2048, 2048, 129), (600, 600, 255),                                   # tap blocks
    (512, 512, 65), (1024, 1024, 127),                                                      # run-time-sized kernels
    (18784, 9256, 33), (16384, 9256, 33),                                                   # the planar mirror's 2 GiB edge
]
SWITCH_DEFAULTS = {"conv_path": 0, "fused_gradk": 1, "fft_gradk": 1, "fft_fused": 1, "small_iter": 1, "planar_image": 1}
SETTINGS = [("default", {})] + [("%s=%d" % (k, v), {k: v}) for k, v in
                                [("conv_path", 1), ("conv_path", 2), ("conv_path", 3), ("fused_gradk", 0), ("fft_gradk", 0),
                                 ("fft_fused", 0), ("small_iter", 0), ("small_iter", 2), ("planar_image", 0)]]
# per shape and setting, one result per combination, in this order (the last one varies fastest)
PARAMS = list(itertools.product((0, 1), (0, 1, 2, 3), (0, 1, 2, 3), (0, 1), (0, 1)))   # blind, conv, tv_mode, fuse, FLAG_NO_FUSED_GRADK
ALPHABET = string.digits + string.ascii_letters + "!#$%&()*+,-./:;<=>?@[]^_{|}~"


def _describe(nv, M, N, MK, blind, conv, tv_mode, fuse, no_fused):
    p = nv.RLJob.params(0, M, 0, N, 1e9, 10, 1e-3, 1e4, blind, tv_mode=tv_mode, conv=conv, fuse=fuse,
                        flags=nv.FLAG_NO_FUSED_GRADK if no_fused else 0)
    try:
        r = nv.describe(M, N, MK, p)
    except nv.NativeError as e:
        return "error %d" % e.code
    return [getattr(r, f) for f, _ in nv.RLRoute._fields_[1:]]


def sweep(set_switch):
    """{setting: {"MxN/K": [result per PARAMS entry]}}; `set_switch(name, value)` sets a debug switch of the library"""
    from lib import _native as nv
    out = {}
    for name, over in SETTINGS:
        for k, v in dict(SWITCH_DEFAULTS, **over).items():
            set_switch(k, v)
        out[name] = {"%dx%d/%d" % s: [_describe(nv, *s, *q) for q in PARAMS] for s in SHAPES}
    return out


def encode(table):
    """one character per result, with a legend: keeps the file to a few tens of KB"""
    legend = []
    for rows in table.values():
        for res in rows.values():
            for x in res:
                if x not in legend:
                    legend.append(x)
    assert len(legend) <= len(ALPHABET), len(legend)
    code = {json.dumps(x): ALPHABET[i] for i, x in enumerate(legend)}
    from lib import _native as nv
    return {"fields": [f for f, _ in nv.RLRoute._fields_[1:]],
            "params": "blind, conv, tv_mode, fuse, FLAG_NO_FUSED_GRADK: itertools.product((0, 1), (0, 1, 2, 3), (0, 1, 2, 3), (0, 1), (0, 1))",
            "legend": {ALPHABET[i]: x for i, x in enumerate(legend)},
            "table": {name: {shape: "".join(code[json.dumps(x)] for x in res) for shape, res in rows.items()} for name, rows in table.items()}}


def test_describe_matches_the_recorded_route_table(debug_switch):
    from lib import _native as nv
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert want["fields"] == [f for f, _ in nv.RLRoute._fields_[1:]]
    got = sweep(debug_switch)
    assert sorted(got) == sorted(want["table"])
    bad = []
    for name, rows in got.items():
        assert sorted(rows) == sorted(want["table"][name])
        for shape, res in rows.items():
            exp = [want["legend"][c] for c in want["table"][name][shape]]
            assert len(exp) == len(res) == len(PARAMS)
            for q, x, y in zip(PARAMS, exp, res):
                if x != y:
                    bad.append("%s %s blind=%d conv=%d tv_mode=%d fuse=%d no_fused=%d: recorded %s, now %s" % ((name, shape) + q + (x, y)))
    assert not bad, "%d of %d routes differ:\n%s" % (len(bad), len(PARAMS) * len(SHAPES) * len(SETTINGS), "\n".join(bad[:30]))
