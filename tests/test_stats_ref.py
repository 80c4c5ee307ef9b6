"""CPU: the references of the stop-test statistics (tests/stats_ref.py) before anything on the device is held against them.

 * reference() against the oracle's own residual_whiteness, direct and scipy convolution, on the small windows
 * separation: on every window of stats_ref.CASES and BIG_CASES each named mutant of the reference -- one lag, weight or scale slip each --
   moves M_r on one of the window's fields by at least 100 x the gate tests/test_gpu_stats_windows.py applies there, unless the mutant
   is an exact symmetry of M_r on that window (stats_ref.exact_symmetry: listed with its reason, and asserted to be one)
 * the noise-like field of the older tests does not separate the lag shifts: why the new fields exist
 * F32_RESTATEMENT_ERROR, the table the GPU gates come from: `python tests/test_stats_ref.py` prints it (all cases, several minutes);
   the suite recomputes the entries of the small transforms"""
import functools
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "oracle"), os.path.join(root, "tests")]
import rl_mm_oracle as orc
import stats_ref as sr

ALL_CASES = sr.CASES + sr.BIG_CASES
# |reference - oracle| / reference of M_r, worst over the windows below: the oracle keeps the normalised window, the autocorrelation, its
# square and the mean in float32 (oracle/rl_mm_oracle.py residual_whiteness).  Measured by `python tests/test_stats_ref.py`.
ORACLE_F32_ERROR = {"direct": 8.316e-07, "scipy": 8.316e-07}
DIRECT_MAX, SCIPY_MAX = 65, 520           # longest side of a window given to the direct / the scipy convolution


def rel(a, b):
    return abs(a - b) / abs(b)


@functools.lru_cache(maxsize=None)
def ref_and_autocorrelation(H, W, gen):
    f = sr.field(gen, H, W, sr.SEED)
    A = sr.autocorrelation64(f)
    return f, A, sr.m_r64(f, A)


def oracle_errors():
    worst = {"direct": 0.0, "scipy": 0.0}
    for c in sr.CASES:
        for gen in c.gens + ("rough",):
            f = sr.field(gen, c.H, c.W, sr.SEED)
            ref = sr.m_r64(f)
            for name, conv, limit in (("direct", orc._conv_direct, DIRECT_MAX), ("scipy", orc._conv_scipy, SCIPY_MAX)):
                if max(c.H, c.W) <= limit:
                    worst[name] = max(worst[name], rel(float(orc.residual_whiteness(f, orc.stop_weights(0, c.H, 0, c.W), conv)), ref))
    return worst


def test_the_cases_reach_the_transform_forms_they_are_there_for():
    assert [c.sizes[0] for c in sr.CASES] == sr.EXPECTED_P
    assert [c.sizes[1:] for c in sr.BIG_CASES] == sr.EXPECTED_PYX and all(c.sizes[0] == 0 for c in sr.BIG_CASES)
    assert sr.MOMENTS.H * sr.MOMENTS.W * 3 > 512 * 256 * 8 and (sr.MOMENTS.H * sr.MOMENTS.W * 3) % (256 * 8) != 0
    C = sr.lines_per_workgroup
    assert {C(P) for P in sr.EXPECTED_P} == {4, 2, 1} and C(2) == 1 and C(4) == 4 and C(1024) == 4 and C(2048) == 2 and C(4096) == 1
    assert [C(min(py, 8192)) for py, _ in sr.EXPECTED_PYX] == [4, 2, 4, 1, 1]
    assert any(c.H % 2 == 0 for c in sr.CASES) and any(c.H % 2 == 1 for c in sr.CASES)
    # 3 H not a multiple of C = 2: a ragged last workgroup in k_fft_mr
    assert any(c.sizes[0] == 2048 and (3 * c.H) % 2 for c in sr.CASES)
    # a grey 1 x 1 window: its deviation is 0 and every reading of pyx:627-638 gives NaN
    one = np.full((1, 1, 3), 0.25, np.float32)
    assert np.isnan(sr.reference(one, one[:0])[0]) and np.isnan(sr.restatement_f32(one, one[:0])[0])


def test_reference_against_the_oracle():
    worst = oracle_errors()
    print("reference against the oracle:", worst)
    for name, err in worst.items():
        assert 0 < ORACLE_F32_ERROR[name] < 5e-6 and err <= 2 * ORACLE_F32_ERROR[name], (name, err)


def case_gate(c):
    """the M_r gate tests/test_gpu_stats_windows.py applies to this window"""
    return sr.gates(c.id)[0]


def separations(c):
    """{mutant: (field that separates it best, relative change of M_r)} for the mutants that are no exact symmetry on this window;
    the exact symmetries are asserted to be exact"""
    out = {}
    for name, mutant in sr.MUTANTS.items():
        why = sr.exact_symmetry(name, c.H, c.W)
        best = ("", 0.0)
        for gen in c.gens:
            f, A, ref = ref_and_autocorrelation(c.H, c.W, gen)
            change = rel(mutant(f, A), ref)
            if why:
                assert change < 1e-9, (c, name, gen, change, why)
            elif change > best[1]:
                best = (gen, change)
            if best[1] >= 1e4 * sr.MR_CAP:      # far past any gate: no need for the other fields
                break
        if not why:
            out[name] = best
    return out


@pytest.mark.parametrize("c", ALL_CASES, ids=repr)
def test_every_mutant_is_separated_from_the_reference(c):
    gate = case_gate(c)
    assert 0 < gate <= sr.MR_CAP
    for name, (gen, change) in separations(c).items():
        print("%s, %s: %s moves M_r by %.3e = %.0f x the gate %.3e" % (c, name, gen, change, change / gate, gate))
        assert change >= 100 * gate, (c, name, gen, change, gate)


def test_no_mutant_is_an_exact_symmetry_on_more_than_a_quarter_of_the_classes():
    """a class is one transform form (stats_ref.Case.klass); a mutant counts as skipped there only if it is an exact symmetry on every
    window of the class.  The long-line scale is counted over the long-line classes: the P x P path has one size and no such slip."""
    for name in sr.MUTANTS:
        cases = sr.BIG_CASES if name.startswith("long-line") else ALL_CASES
        classes = sorted({c.klass for c in cases})
        skipped = [k for k in classes if all(sr.exact_symmetry(name, c.H, c.W) for c in cases if c.klass == k)]
        print("%s: skipped on %d of %d classes %s" % (name, len(skipped), len(classes), skipped))
        assert 4 * len(skipped) <= len(classes), (name, skipped)


@pytest.mark.parametrize("H,W", [(256, 300), (512, 513)])
def test_a_noise_field_does_not_separate_the_lag_shifts(H, W):
    """on the field of the older tests one lag row or column off stays below their gate of 2e-4, and below 100 x the gate a pair field of
    the same size gets here: neither the old gate nor the new one could tell the shift from rounding"""
    f = sr.field("rough", H, W, sr.SEED)
    A = sr.autocorrelation64(f)
    ref = sr.m_r64(f, A)
    new_gate = sr.gates("257x256")[0]
    for name in ("lag row +1", "lag row -1", "lag column +1"):
        change = rel(sr.MUTANTS[name](f, A), ref)
        print("rough %d x %d, %s: %.3e" % (H, W, name, change))
        assert change < sr.MR_CAP and change < 100 * new_gate, (name, change)


def restatement_errors(c, gen):
    if c is sr.MOMENTS:
        e, u = sr.moments_frames()
        f = e[c.win[0]:c.win[1], c.win[2]:c.win[3]]
    else:
        f, u = sr.field(gen, c.H, c.W, sr.SEED), c.u_frame()
    uw = c.u_window(u)
    ref, r32 = sr.reference(f, uw), sr.restatement_f32(f, uw)
    return tuple(rel(a, b) if b == b else float("nan") for a, b in zip(r32, ref))


def on_cpu(c):
    """which fields of a case the suite restates: all of them for transforms up to 256 x 256 points, `pairs` alone up to 2^21"""
    n = c.sizes[0] ** 2 or c.sizes[1] * c.sizes[2]
    return c.gens if n <= 1 << 16 else (c.gens[:1] if n <= 1 << 21 else ())


def test_the_table_has_every_case_and_no_gate_is_above_the_present_ones():
    want = {(c.id, gen) for c in ALL_CASES + [sr.MOMENTS] for gen in c.gens}
    assert set(sr.F32_RESTATEMENT_ERROR) == want
    for key, entry in sr.F32_RESTATEMENT_ERROR.items():
        g = sr.gates(key[0])
        assert 0 < entry[0] and g[0] <= sr.MR_CAP and 0 <= entry[1] and g[1] <= sr.HU_CAP and (entry[2] != entry[2] or g[2] <= sr.HU_CAP), key


@pytest.mark.parametrize("c", [c for c in ALL_CASES if on_cpu(c)], ids=repr)
def test_recorded_restatement_errors(c):
    for gen in on_cpu(c):
        got, want = restatement_errors(c, gen), sr.F32_RESTATEMENT_ERROR[c.id, gen]
        for g, w in zip(got, want):
            assert (g != g and w != w) or abs(g - w) <= 2e-3 * w + 1e-12, (c, gen, got, want)     # four printed digits


if __name__ == "__main__":
    print("ORACLE_F32_ERROR = {%s}" % ", ".join('"%s": %.3e' % kv for kv in oracle_errors().items()))
    print("F32_RESTATEMENT_ERROR = {")
    for c in ALL_CASES + [sr.MOMENTS]:
        for gen in c.gens:
            print('    ("%s", "%s"): (%s),' % (c.id, gen, ", ".join("%.3e" % v if v == v else 'float("nan")' for v in restatement_errors(c, gen))), flush=True)
    print("}")
    if sr.F32_RESTATEMENT_ERROR:
        for c in ALL_CASES:
            gate = case_gate(c)
            print("%s (gate %.2e): " % (c, gate) + "; ".join("%s: %s %.2e" % (n, g, ch) for n, (g, ch) in separations(c).items()), flush=True)
