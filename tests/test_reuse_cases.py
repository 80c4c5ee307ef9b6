"""tests/reuse_cases.py without a device: every run kind reaches the route it claims, every piece of state a job carries between calls has
a kind that owns it, and the two pictures of a shape differ almost everywhere."""
import numpy as np
import pytest

import reuse_cases as ru


@pytest.mark.parametrize("kind", ru.KINDS, ids=lambda k: k.id)
def test_kind_reaches_the_route_it_claims(kind):
    before = ru.switch_values()
    with ru.switches_set(kind):
        inside = ru.switch_values()
    assert inside == dict(ru.SWITCH_DEFAULTS, key_trace=1, **dict(kind.switches))
    assert ru.describe(kind) == kind.route
    assert ru.switch_values() == before         # every switch is back where it was


def test_switch_table_holds_the_librarys_defaults():
    """(csrc/ics_common.h IcsDebug; every test that sets a switch puts it back)"""
    assert ru.switch_values() == ru.SWITCH_DEFAULTS


def test_kinds_differ_from_the_default_route_where_their_switch_says_so():
    """a switch that does nothing would make its kind a copy of another: each of these pairs must differ in what describe reports"""
    by = ru.BY_ID
    for a, b in (("mx-fused", "mx-nofused"), ("mx-fused", "mx-planar0"), ("mx-nb", "mx-nb-rs"), ("mx-fused", "mx-fuse1"), ("ti-bl", "ti-bl-two"),
                 ("ti-bl", "ti-bl-gk0"), ("small", "mx-fused"), ("vec-bl", "mx-nofused"), ("blk-bl", "vec51-bl"), ("ti87-bl", "blk87-bl"),
                 ("blk87-bl", "vec87-bl"), ("mx-fused", "tv1-mx")):
        assert ru.describe(by[a]) != ru.describe(by[b]), (a, b)


def test_every_state_item_has_an_owner():
    owned = {}
    for k in ru.KINDS:
        assert set(k.owns) <= set(ru.STATE), k.id
        for letter in k.owns:
            owned.setdefault(letter, []).append(k.id)
    assert sorted(owned) == sorted(ru.STATE), sorted(set(ru.STATE) - set(owned))
    # the owners are of the family that builds the piece
    fam = {k.id: k.route[0] for k in ru.KINDS}
    assert all(fam[i] == ru.MATRIX for i in owned["a"]) and all(fam[i] == ru.BLOCKS for i in owned["b"] + owned["g"])
    assert all(fam[i] == ru.TILES for i in owned["c"] + owned["d"] + owned["e"] + owned["i"] + owned["l"])
    assert {fam[i] for i in owned["h"]} == {ru.SMALL, ru.MATRIX}
    assert all(ru.BY_ID[i].tv_mode for i in owned["j"]) and all(ru.BY_ID[i].fuse for i in owned["m"])
    assert all(ru.BY_ID[i].switch("fft_maxg") == 2 for i in owned["i"])
    assert all(ru.SHAPES[ru.BY_ID[i].shape][2] <= 25 and ru.BY_ID[i].switch("fft_conv2") for i in owned["d"])      # (route_cases.CONV2_MAX_K)
    assert {k.switch("conv_rs") for k in ru.KINDS if "a" in k.owns} >= {0, 2} and any(k.switch("fused_rs") == 4 for k in ru.KINDS if "a" in k.owns)


def test_mode2_units_that_read_the_image_spectra():
    """fspec is read by the mode-2 units whose two tiles lie inside the image: none on S1, some on S4 -- the kinds that own row d there are the ones
    that can see a stale fspec.  The restated tile grid gives the unit count the library reports."""
    from lib import _native as nv
    for s in ("S1", "S4"):
        assert 3 * len(ru.mode2_pairs(s)) == nv.conv2_units(*ru.SHAPES[s]), s
    assert all(ru.mode2_pairs("S1")) and len(ru.mode2_pairs("S1")) == 5
    assert ru.mode2_pairs("S4").count(False) >= 1 and len(ru.mode2_pairs("S4")) == 8
    assert any("d" in k.owns and k.blind for k in ru.kinds("S4")) and any("d" in k.owns and not k.blind for k in ru.kinds("S4"))
    assert any("d" in ru.BY_ID[i].owns and ru.BY_ID[i].shape == "S4" for i in ru.IMAGE_COPY)


def test_lists_name_kinds_of_the_right_shape():
    assert len(ru.kinds("S1")) >= 20 and len(ru.kinds("S2")) >= 5 and len(ru.kinds("S3")) >= 3
    for i in ru.FIXED_B + ru.SPECIAL_A + ru.STAGE_A:
        assert ru.BY_ID[i].shape == "S1"
    for i in ru.IMAGE_COPY:
        assert set(ru.BY_ID[i].owns) & set("abcd"), i
        assert ru.BY_ID[i].shape in ru.IMAGE_STEPPER
    for s, i in ru.IMAGE_STEPPER.items():
        assert ru.BY_ID[i].shape == s and ru.BY_ID[i].tv_mode == 1
    assert {ru.BY_ID[i].route[0] for i in ru.READ_KINDS} == {ru.MATRIX, ru.BLOCKS, ru.PACKED, ru.SIZED, ru.TILES, ru.SMALL}
    assert all(ru.BY_ID[i].tv_mode == 0 for i in ru.READ_KINDS)
    assert ru.ROWS[0] > 0 and ru.ROWS[0] + ru.ROWS[1] < min(ru.SHAPES[s][0] for s in ru.SHAPES)


def test_a_iterations_reach_all_three_counts_for_every_kind():
    for s in ru.SHAPES:
        n = len(ru.kinds(s))
        for ia in range(n):
            assert {ru.a_iterations(s, ia, ib) for ib in range(n)} == {1, 2, 3}, (s, ia)


@pytest.mark.parametrize("shape", sorted(ru.SHAPES))
def test_the_two_pictures_differ_almost_everywhere(shape):
    d = ru.data(shape)
    M, N, MK = ru.SHAPES[shape]
    for name in ("image", "u"):
        a, b = d["a"][name], d["b"][name]
        assert a.shape == b.shape == ((M, N, 3) if name == "image" else (M + MK - 1, N + MK - 1, 3)) and a.dtype == b.dtype == np.float32
        assert np.mean(a != b) > 0.99, (name, float(np.mean(a != b)))
        assert not a.flags.writeable and not b.flags.writeable
    assert float(d["b"]["image"].max()) < 0.75 * 0.95        # (scaled by 0.7: the recipe's scenes stay below 0.95)
    psfs = [d[x][y] for x in "ab" for y in ("psf_blind", "psf_true")]
    for i, p in enumerate(psfs):
        assert np.allclose(p.sum(axis=(0, 1), dtype=np.float64), 1.0, atol=1e-4) and p.min() >= 0
        for q in psfs[i + 1:]:
            assert np.abs(p - q).max() > 1e-2 * max(p.max(), q.max())
