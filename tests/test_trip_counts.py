"""CPU: the shapes of the GPU tests that are there to take a kernel past its first trip or its first chunk do so, by the kernels' own
constants.  tests/trips_ref.py reads the #defines from csrc/ and restates each launcher's grid rule for 256 CUs (what csrc/ics_route.hip
assumes without a device); a constant or a rule that changes fails here instead of silently turning these cases back into one-trip
cases.  The GPU tests assert the same conditions on the device's own CU count where that count matters."""
import align_ref as ar
import mask_ref as mr
import test_mask as tm
import trips_ref as tr


def test_the_constants_the_arithmetic_rests_on():
    assert tr.defines("ics_img_align.hip", "ALT", "ALRED") == (ar.TILE, 1024)
    assert tr.defines("ics_img_mask.hip", "MKPICK", "MKCELL") == (1024, mr.CELL)
    assert tr.defines("ics_img_edges.hip", "EDLANES", "EDHK") == (256, 4)
    assert tr.defines("ics_img_noise.hip", "NSLANES", "NSHK", "NSTW", "NSTH") == (256, 4, 64, 16)
    assert tr.grid_cap() == (65536, 256)
    for unit in ("ics_img_edges.hip", "ics_img_noise.hip"):          # without a CU count the launchers assume tr.CUS
        assert "cus > 0 ? cus : 256" in tr.source(unit), unit
    assert tr.CUS == 256
    # the loops themselves, as the restatements read them
    assert "for (; t + 7 * parts < tiles; t += 8 * parts)" in tr.source("ics_img_align.hip") and "const int parts = ALRED / ns" in tr.source("ics_img_align.hip")
    assert "for (; c + 7 * MKPICK < cand; c += 8 * MKPICK)" in tr.source("ics_img_mask.hip")
    for unit in ("ics_img_edges.hip", "ics_img_noise.hip"):          # the switch that lets two workgroups, or one, walk a small frame
        assert "ics_debug().max_wgs" in tr.source(unit), unit


def test_align_cases_run_both_loop_forms_of_the_reduction():
    assert [tr.align_slot_floats(ar.MODELS[m] + 2 * p) for m in ar.MODELS for p in (0, 1)] == [7, 16, 29, 46, 46, 67]
    seen = set()
    for shape, model, photometric in ar.SUMS_TRIP_CASES[:-1]:
        n = ar.MODELS[model] + (2 if photometric else 0)
        parts, tiles = 1024 // tr.align_slot_floats(n), tr.align_tiles(*shape)
        forms = tr.align_reduce_forms(*shape, n)
        print(shape, model, photometric, "ns", tr.align_slot_floats(n), "parts", parts, "tiles", tiles, forms)
        assert 8 * parts < tiles < 9 * parts
        assert forms == {(1, 1): tiles - 8 * parts, (1, 0): 9 * parts - tiles}          # every lane one eight-wide trip, some a tail step too
        seen.add((model, photometric))
    assert seen == {(m, p) for m in ar.MODELS for p in (True, False)}                   # every variant
    shape, model, photometric = ar.SUMS_TRIP_CASES[-1]                                  # the many-trip case: the widest variant, the largest frame
    assert (model, photometric) == ("homography", True) and tr.align_tiles(*shape) == 1190
    forms = tr.align_reduce_forms(*shape, 10)
    assert forms == {(10, 0): 5, (9, 7): 10} and sum(forms.values()) == 1024 // 67      # ten trips, or nine and a tail of seven
    # the cases from before stay below the first eight-wide trip: both forms are tested, neither replaced the other
    for shape_f, _, window in ar.SUMS_CASES:
        H, W = shape_f if window is None else (window[1] - window[0], window[3] - window[2])
        assert all(trips == 0 for n in (2, 4, 6, 8, 10) for trips, _ in tr.align_reduce_forms(H, W, n))


def test_mask_pick_cases_sit_in_the_lane_classes_they_name():
    for side, cand in ((1360, mr.grid((0, 1360, 0, 1360), 16)), (tm.PICK_SIDE, mr.grid((0, tm.PICK_SIDE, 0, tm.PICK_SIDE), 16))):
        assert cand == (1, 0, 85, 85), side
    cand, lanes = tm.PICK_N ** 2, 1024
    assert 7 * lanes < cand < 8 * lanes
    wide = cand - 7 * lanes                                                              # lanes below: one eight-wide trip, no tail
    assert tr.pick_forms(cand) == {(1, 0): wide, (0, 7): lanes - wide} and wide == 57
    eight = lambda c: c % lanes < wide                                                   # noqa: E731
    cases = tm.PICK_CASES
    assert eight(cases["eight-wide, first slot"][0]) and cases["eight-wide, first slot"][0] // lanes == 0
    assert eight(cases["eight-wide, fourth slot"][0]) and cases["eight-wide, fourth slot"][0] // lanes == 3
    assert not eight(cases["tail only"][0])
    a, b = cases["a tie, the eight-wide lane first"]
    assert a < b and eight(a) and not eight(b)
    a, b = cases["a tie, the tail-only lane first"]
    assert a < b and not eight(a) and eight(b)
    for raised in cases.values():                                                        # raised cells never touch: their ties are exact
        cells = [divmod(c, tm.PICK_N) for c in raised]
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) > 1 for p in cells for q in cells if p != q)
    # the largest candidate table of the tests from before: all tail
    assert tr.pick_forms(15 * 15) == {(0, 1): 225, (0, 0): lanes - 225}


def test_the_large_frame_exceeds_every_cap_and_the_small_ones_none():
    H, W = tr.BIG
    assert (H, W) == (1030, 1100) == tr.past_the_caps(256) and H % 4 and H % 16 and W % 64
    assert H * W / 1024 > 4 * 256 and tr.ceil_div(H, 4) * tr.ceil_div(W, 64) > 8 * 256   # key units against the "vector" count cap, tiles against the mask cap
    for coupling in ("channel", "vector"):
        for route in (1, 2):
            for grids in (tr.edge_mask_grids(H, W, coupling, route), tr.noise_grids(H, W, coupling, route)):
                for kernel, (units, cap) in grids.items():
                    print(coupling, route, kernel, units, cap)
                    assert units > cap, (kernel, units, cap)
    assert tr.edge_mask_grids(H, W, "vector", 2) == {"k_img_ed_keys": (4644, 1024), "k_img_ed_hist": (1107, 1024), "k_img_ed_mask_keys": (4426, 2048)}
    assert tr.noise_grids(H, W, "vector", 2) == {"k_img_ns_keys": (1170, 1024), "k_img_ns_hist": (1107, 1024)}
    assert tr.noise_grids(H, W, "channel", 2) == {"k_img_ns_keys": (1170, 512), "k_img_ns_hist": (1107, 1024)}
    # a device with more CUs gets a larger frame, which still exceeds them
    for cus in (304, 512):
        h, w = tr.past_the_caps(cus)
        assert all(u > c for coupling in ("channel", "vector") for route in (1, 2)
                   for g in (tr.edge_mask_grids(h, w, coupling, route, cus), tr.noise_grids(h, w, coupling, route, cus)) for u, c in g.values())
    # what the max_wgs cases are for: on the frames from before, route 2 of the noise estimate and the edge mask stay below their caps
    assert all(u <= c for coupling in ("channel", "vector") for u, c in tr.noise_grids(700, 513, coupling, 2).values())
    assert tr.noise_grids(700, 513, "vector", 2) == {"k_img_ns_keys": (396, 1024), "k_img_ns_hist": (351, 1024)}
    assert all(u <= c for coupling in ("channel", "vector") for route in (1, 2) for u, c in tr.edge_mask_grids(70, 150, coupling, route).values())
    for shape in ((70, 150), (301, 287)):                                                # ... and with one or two workgroups everything wraps
        assert all(u > 2 for coupling in ("channel", "vector") for route in (1, 2)
                   for g in (tr.edge_mask_grids(*shape, coupling, route), tr.noise_grids(*shape, coupling, route)) for u, _ in g.values())


def test_the_stride_frame_takes_a_second_step_and_no_third():
    cap, lanes = tr.grid_cap()
    H, W = tr.STRIDE_FRAME
    assert cap * lanes == 16777216 < H * W * 3 == 16822272 < 2 * cap * lanes
    assert 37 * 45 * 3 < cap * lanes                                                     # the frame of the test from before: one step
