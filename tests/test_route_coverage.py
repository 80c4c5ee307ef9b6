"""Every kernel route resolve_route can pick has a whole-call case in tests/route_cases.py (CPU only: ics_describe needs no device).

tests/test_route_table.py pins which route each shape and parameter set takes; tests/test_gpu_route_matrix.py runs the cases of
tests/route_cases.py against the oracle.  This file checks that the two meet: a route of tests/golden/route_table.json that no case
reaches -- a new family added to resolve_route without a numerical test, say -- fails here, and names the route."""
import collections

import route_cases as rc


def _routes_by_tv():
    got = collections.defaultdict(set)
    R = rc.routes()
    for c in rc.cases():
        if c.id not in rc.EXCLUDED:          # (cases the GPU matrix does not compare are no coverage)
            got[c.tv_mode].add(R[c.id])
    return got


def test_print_route_to_cases():
    leg = {v: k for k, v in rc.legend().items()}
    for r, ids in sorted(rc.route_map().items()):
        print("%s %s %3d cases: %s" % (r, list(leg[r]), len(ids), " ".join(ids)))


def test_every_route_of_the_shipped_loop_has_a_case():
    want, got = rc.table_routes()[0], _routes_by_tv()[0]
    leg = {v: k for k, v in rc.legend().items()}
    missing = sorted(want - got)
    assert not missing, "routes of tv_mode 0 without a case in tests/route_cases.py: %s" % ", ".join("%s %s" % (r, list(leg[r])) for r in missing)


def test_every_route_of_each_tv_mode_has_a_case():
    want, got = rc.table_routes(), _routes_by_tv()
    leg = {v: k for k, v in rc.legend().items()}
    missing = ["tv_mode %d: %s %s" % (m, r, list(leg[r])) for m in (1, 2, 3) for r in sorted(want[m] - got[m])]
    assert not missing, "routes without a case of that tv_mode: %s" % "; ".join(missing)


def test_every_route_of_every_tv_mode_has_a_cheapest_case():
    """rc.cheapest_per_route, the whole calls tests/test_gpu_pool_check.py repeats on poisoned pool blocks: one per route of the table and
    tv_mode, and it is the cheapest of its route"""
    pick = rc.cheapest_per_route()
    want = rc.table_routes()
    leg = {v: k for k, v in rc.legend().items()}
    missing = ["tv_mode %d: %s %s" % (m, r, list(leg[r])) for m in range(4) for r in sorted(want[m]) if (m, r) not in pick]
    assert not missing, "routes without a case of that tv_mode: %s" % "; ".join(missing)
    R = rc.routes()
    cost = lambda c: c.M * c.N * c.MK ** 2 * c.iters
    for (m, r), c in pick.items():
        assert c.tv_mode == m and R[c.id] == r and c.id not in rc.EXCLUDED
        assert all(cost(c) <= cost(o) for o in rc.cases() if o.tv_mode == m and R[o.id] == r and o.id not in rc.EXCLUDED), c.id
    print("%d whole calls: %s" % (len(pick), " ".join("%d%s:%s" % (m, r, c.id) for (m, r), c in sorted(pick.items()))))


def test_the_list_holds_every_switch_and_variant():
    cs = [c for c in rc.cases() if c.id not in rc.EXCLUDED]
    R = rc.routes()
    leg = {v: k for k, v in rc.legend().items()}
    fam = lambda c: leg[R[c.id]][0]
    need = {
        "fuse = 1": [c for c in cs if c.fuse],
        "fft_conv2 = 0": [c for c in cs if c.switch("fft_conv2") == 0 and fam(c) == 5],
        "fft_conv2 = 2": [c for c in cs if c.switch("fft_conv2") == 2 and fam(c) == 5],
        "fft_rot = 0": [c for c in cs if c.switch("fft_rot") == 0 and fam(c) == 5],
        "planar_image = 0": [c for c in cs if c.switch("planar_image") == 0],
        "fused_rs = 2": [c for c in cs if c.switch("fused_rs") == 2 and leg[R[c.id]][2] == 1],
        "fused_rs = 4": [c for c in cs if c.switch("fused_rs") == 4 and leg[R[c.id]][2] == 1],
        "small max_wgs": [c for c in cs if 0 < c.switch("max_wgs") <= 8],
        "an ICS_CONV_AUTO case": [c for c in cs if c.conv == 0 and not c.switches],
    }
    for f in (1, 2, 3, 4, 5, 6):
        need["correlation = 1 on conv family %d" % f] = [c for c in cs if c.correlation and fam(c) == f]
    for v in rc.VARIANTS:
        need["data variant %s" % v] = [c for c in cs if c.variant[0] == v]
    missing = [k for k, v in need.items() if not v]
    assert not missing, missing


def test_excluded_cases_exist():
    assert rc.EXCLUDED <= {c.id for c in rc.cases()}


def test_cases_are_deterministic_and_in_bounds():
    a = [(c.id, c.seed, c.win, c.variant) for c in rc._build()]
    assert a == [(c.id, c.seed, c.win, c.variant) for c in rc.cases()]
    for c in rc.cases():
        t, b, l, r = c.win
        assert 0 <= t < b <= c.M and 0 <= l < r <= c.N, c.id
        assert c.MK % 2 == 1 and 3 <= c.MK <= 255, c.id
        if c.variant[0] in ("black_top", "black_bottom"):
            assert 1 <= c.variant[1] < c.M, c.id
        if c.variant[0] == "black_left":
            assert 1 <= c.variant[1] < c.N, c.id
