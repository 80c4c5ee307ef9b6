"""CPU: the float64 oracle of tests/mask_ref.py (the specification of csrc/ics_img_mask.hip) against a literal triple loop, the cell
and candidate arithmetic, what the score is for on "dead leaves" frames (tests/test_blur_width.py dead_leaves), the argument handling
of lib._native.window_scores_args, lib.utils.best_mask and deblur_module(mask=...), and the header and export of the C entry.

Property frames, 160 x 192 with a box of 63 (n = 3, off = 7):
  (a) a sharp 80 x 80 patch pasted into the box-9-blurred frame of the same seed: the chosen box lies inside the patch;
  (b) the left half replaced by hard horizontal stripes: the largest trace by far and one orientation only -- every box wholly in the
      stripes scores below 5 % of the best;
  (c) a 96 x 96 checker of 1.0 / 0.2 in the top left corner: with clip 0.99 its 1.0 pixels are unusable and its 0.2 pixels flat, the
      choice and its score are those of the frame without the checker, and no chosen cell is clipped; with clip = inf the checker wins.
The seeds are chosen so that the float64 oracle ALONE meets these (a condition on the inputs, re-asserted here) and so that the best
candidate beats the second by at least 100 x the gate of tests/test_gpu_mask.py: float32 cannot flip a choice."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import mask_ref as mr
from test_blur_width import dead_leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, BOX = 160, 192, 63
SEEDS = (109, 115)                  # of 100 .. 134, the first two that meet the conditions of test_properties_on_dead_leaves
PATCH = (32, 112, 32, 112)          # (a): rows and columns of the sharp patch
CHECKER = 96                        # (c): side of the checker, squares of 8


@functools.lru_cache(maxsize=None)
def frame(seed, kind):
    """the property frames: "blurred" (the box-9 frame itself), "patch", "stripes", "checker" """
    f = np.array(dead_leaves(seed, H, W, "box", 9))
    if kind == "patch":
        y0, y1, x0, x1 = PATCH
        f[y0:y1, x0:x1] = dead_leaves(seed, H, W)[y0:y1, x0:x1]
    elif kind == "stripes":
        rng = np.random.default_rng(seed + 5000)
        rows = np.where((np.arange(H) // 2) % 2 == 0, 0.2, 0.8)
        f[:, :W // 2] = (rows[:, None, None] + rng.normal(0.0, 0.01, (H, W // 2, 3))).astype(np.float32)
    elif kind == "checker":
        y, x = np.mgrid[:CHECKER, :CHECKER]
        f[:CHECKER, :CHECKER] = np.where(((y // 8 + x // 8) % 2 == 0)[..., None], np.float32(1.0), np.float32(0.2))
    elif kind != "blurred":
        raise ValueError(kind)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle(seed, kind, clip=0.99):
    """(score, trace, clipped) maps of the float64 oracle on the whole frame, computed once"""
    return mr.scores(frame(seed, kind), (0, H, 0, W), BOX, clip, np.float64)


def lead(score, trace):
    """(best - second best score, trace of the best): the room a choice has"""
    flat = np.sort(score.ravel())
    at = np.unravel_index(int(np.argmax(score)), score.shape)
    return float(flat[-1] - flat[-2]), float(trace[at])


def test_oracle_against_a_literal_triple_loop():
    rng = np.random.default_rng(11)
    pic = rng.random((40, 50, 3)).astype(np.float32)
    pic[rng.random((40, 50)) < 0.05, 1] = 1.0                     # unusable at clip 0.99
    pic[9, 13, 0], pic[20, 30, 2] = np.nan, np.inf
    region, size, clip = (3, 39, 5, 48), 17, 0.99                 # n = 1, off = 0, 2 x 2 candidates; an odd origin
    y0, y1, x0, x1 = region
    score, trace, bad = mr.scores(pic, region, size, clip)
    assert score.shape == trace.shape == bad.shape == (2, 2) and bad.dtype == np.int64
    p = pic.astype(np.float64)
    ok = lambda y, x: all(abs(p[y, x, k]) < np.float32(clip) for k in range(3))
    luma = lambda y, x: (p[y, x, 0] + p[y, x, 1] + p[y, x, 2]) * (1.0 / 3.0)
    for i in range(2):
        for j in range(2):
            sxx = syy = sxy = 0.0
            count = 0
            for y in range(y0 + 16 * i, y0 + 16 * i + 16):
                for x in range(x0 + 16 * j, x0 + 16 * j + 16):
                    dx = luma(y, x + 1) - luma(y, x) if x + 1 < x1 and ok(y, x) and ok(y, x + 1) else 0.0
                    dy = luma(y + 1, x) - luma(y, x) if y + 1 < y1 and ok(y, x) and ok(y + 1, x) else 0.0
                    sxx, syy, sxy, count = sxx + dx * dx, syy + dy * dy, sxy + dx * dy, count + (not ok(y, x))
            want = max(0.0, 0.5 * (sxx + syy - math.sqrt((sxx - syy) ** 2 + 4.0 * sxy * sxy)) / 256.0)
            assert score[i, j] == pytest.approx(want, rel=1e-11) and trace[i, j] == pytest.approx((sxx + syy) / 256.0, rel=1e-12)
            assert bad[i, j] == count and count > 0
    assert np.isfinite(score).all() and score.min() > 0
    # the float32 restatement: the same counts, scores within float32 rounding of the oracle
    s32, t32, b32 = mr.scores(pic, region, size, clip, np.float32)
    assert b32.tolist() == bad.tolist() and s32.dtype == t32.dtype == np.float64
    assert np.abs(s32 - score).max() <= 1e-6 * trace.max() and np.abs(t32 - trace).max() <= 1e-6 * trace.max()
    # clip = inf keeps every finite pixel: only the NaN and the inf are left out
    assert mr.scores(pic, region, size, np.inf)[2].sum() == 2


def test_cell_and_candidate_arithmetic():
    assert mr.CELL == 16 and mr.TILE % mr.CELL == 0
    assert mr.grid((0, 31, 0, 31), 31) == (1, 7, 1, 1)
    assert mr.grid((0, 16, 0, 16), 16) == (1, 0, 1, 1) and mr.grid((0, 33, 0, 49), 17) == (1, 0, 2, 3)
    assert mr.grid((5, 306, 7, 294), 63) == (3, 7, 15, 15) and mr.grid((0, 301, 0, 287), 255) == (15, 7, 3, 3)
    assert mr.grid((0, 4096, 0, 4096), 1023) == (63, 7, 193, 193)
    for region, size, word in (((0, 30, 0, 31), 31, "smaller"), ((0, 31, 0, 30), 31, "smaller"), ((0, 31, 0, 31), 15, "size")):
        with pytest.raises(ValueError, match=word):
            mr.grid(region, size)
    # size 31 on 47 x 47: off = 7, so box (1, 1) is scored over the pixels 23 .. 38 and no others
    pic = np.full((47, 47, 3), 0.5, np.float32)
    pic[30, 30] = 0.25
    score, trace, bad = mr.scores(pic, (0, 47, 0, 47), 31, 0.99)
    assert score.shape == (2, 2) and (trace > 0).tolist() == [[False, False], [False, True]]
    pic[30, 30] = 0.5
    pic[22, 30] = 0.25                                            # one row above that cell: a difference belongs to its upper (left) pixel
    assert not mr.scores(pic, (0, 47, 0, 47), 31, 0.99)[1][1, 1]
    # a constant frame and a wholly clipped one: every score 0, the tie goes to (0, 0)
    for value in (0.5, 1.0):
        flat = np.full((70, 90, 3), value, np.float32)
        assert mr.choice(flat, (0, 70, 0, 90), 33, 0.99) == (0, 0, 0.0, 0.0, 1024 if value == 1.0 else 0)
    # ... and between equal maxima the lowest i, then the lowest j: two identical textures, far apart
    rng = np.random.default_rng(5)
    tex = rng.random((16, 16, 3)).astype(np.float32) * 0.9
    pic = np.full((80, 80, 3), 0.5, np.float32)
    for y, x in ((32, 48), (32, 16), (48, 0)):
        pic[y:y + 16, x:x + 16] = tex
    score, _, _ = mr.scores(pic, (0, 80, 0, 80), 16, 0.99)
    assert score[2, 3] == score[2, 1] == score.max() and mr.choice(pic, (0, 80, 0, 80), 16, 0.99)[:2] == (2, 1)


# ---- exact ties over many candidates: the pictures of tests/test_gpu_mask.py's pick test ---------------------------------------------------
# One 16 x 16 texture repeated over 1361 x 1361 (85 periods and the pixel that completes the last cells' differences): with a box of 16 a
# candidate is one cell, 85 x 85 = 7225 of them, and every cell sees the same numbers in the same places, so all scores are one and the
# same bits.  Raising the texture's contrast in the cell of candidate c makes that cell the maximum; two raised cells that do not touch
# tie exactly.  k_img_mk_pick (1024 lanes, eight candidates a trip while c + 7 * 1024 < cand, then one at a time) gives lanes 0 .. 56 one
# eight-wide trip and no tail, lanes 57 .. 1023 seven tail steps: the cases put a maximum in each class and a tie across them, both ways round.
PICK_SIDE, PICK_N = 85 * 16 + 1, 85
PICK_CASES = {"eight-wide, first slot": (23,), "eight-wide, fourth slot": (3 * 1024 + 31,), "tail only": (3450,),
              "a tie, the eight-wide lane first": (3 * 1024 + 31, 3450), "a tie, the tail-only lane first": (500, 3 * 1024 + 31)}


def pick_picture(raised=()):
    """the periodic picture, the cells of the candidates `raised` at three times the contrast; float32, 1361 x 1361 x 3"""
    tex = np.random.default_rng(77).random((16, 16, 3)) - 0.5
    base, strong = (0.5 + 0.1 * tex).astype(np.float32), (0.5 + 0.3 * tex).astype(np.float32)
    pic = np.tile(base, (PICK_N + 1, PICK_N + 1, 1))[:PICK_SIDE, :PICK_SIDE]
    for c in raised:
        i, j = divmod(c, PICK_N)
        pic[16 * i:16 * i + 16, 16 * j:16 * j + 16] = strong
    return np.ascontiguousarray(pic)


def test_the_pick_pictures_tie_exactly_and_put_the_maximum_where_they_say():
    whole = (0, PICK_SIDE, 0, PICK_SIDE)
    assert mr.grid(whole, 16) == (1, 0, PICK_N, PICK_N)
    score, trace, bad = mr.scores(pick_picture(), whole, 16, 0.99)
    assert score.min() == score.max() > 0 and not bad.any() and mr.choice(pick_picture(), whole, 16, 0.99)[:2] == (0, 0)
    plain = score[0, 0]
    for name, raised in PICK_CASES.items():
        score, trace, bad = mr.scores(pick_picture(raised), whole, 16, 0.99)
        flat = score.ravel()
        top = np.flatnonzero(flat == flat.max())
        print("%s: maxima at %s, %.3e against %.3e elsewhere at most" % (name, top.tolist(), flat.max(), np.delete(flat, top).max()))
        assert top.tolist() == sorted(raised) and int(np.argmax(flat)) == min(raised), name
        assert np.delete(flat, top).max() < 0.5 * flat.max() and flat.max() > 4 * plain, name
        assert mr.choice(pick_picture(raised), whole, 16, 0.99)[:2] == divmod(min(raised), PICK_N), name


@pytest.mark.parametrize("seed", SEEDS)
def test_properties_on_dead_leaves(seed):
    """what the score is for, by the float64 oracle alone"""
    import test_gpu_mask as tg
    room = 100 * 4 * tg.F32_RESTATEMENT_ERROR
    # (a) the sharp patch
    score, trace, bad = oracle(seed, "patch")
    i, j = np.unravel_index(int(np.argmax(score)), score.shape)
    y0, y1, x0, x1 = PATCH
    gap, tr = lead(score, trace)
    print("seed %d (a): box origin (%d, %d), score %.3e, lead %.3e = %.2e of the trace" % (seed, 16 * i, 16 * j, score[i, j], gap, gap / tr))
    assert y0 <= 16 * i and 16 * i + BOX <= y1 and x0 <= 16 * j and 16 * j + BOX <= x1
    assert gap >= room * tr
    # (b) the stripes
    score, trace, bad = oracle(seed, "stripes")
    inside = [(a, b) for a in range(score.shape[0]) for b in range(score.shape[1]) if 16 * b + BOX <= W // 2]
    assert len(inside) == 3 * score.shape[0]
    worst = max(score[c] for c in inside)
    outside = np.array([[16 * b >= W // 2 for b in range(score.shape[1])]] * score.shape[0])
    gap, tr = lead(score, trace)
    print("seed %d (b): stripes score at most %.3e of the best, trace at least %.1f x any other" % (seed, worst / score.max(), min(trace[c] for c in inside) / trace[outside].max()))
    assert worst < 0.05 * score.max() and min(trace[c] for c in inside) > trace[outside].max()
    assert 16 * np.unravel_index(int(np.argmax(score)), score.shape)[1] + BOX > W // 2 and gap >= room * tr
    # (c) the clipped checker
    plain, checker, blind = oracle(seed, "blurred"), oracle(seed, "checker"), oracle(seed, "checker", np.inf)
    at = np.unravel_index(int(np.argmax(plain[0])), plain[0].shape)
    assert np.unravel_index(int(np.argmax(checker[0])), checker[0].shape) == at and checker[0][at] == plain[0][at] and checker[2][at] == 0
    assert max(16 * at[0], 16 * at[1]) >= CHECKER + 1                        # (the chosen box has no pixel in common with the checker)
    assert checker[0][:3, :3].max() < 0.05 * checker[0][at] and checker[2][0, 0] == 48 * 48 // 2
    gap, tr = lead(checker[0], checker[1])
    print("seed %d (c) clip 0.99: lead %.3e = %.2e of the trace" % (seed, gap, gap / tr))
    assert gap >= room * tr
    # clip = inf: the nine boxes wholly in the checker hold the same cells (16 px is its period) and tie exactly: (0, 0) wins, far ahead
    win = np.unravel_index(int(np.argmax(blind[0])), blind[0].shape)
    rest = np.array(blind[0])
    rest[:3, :3] = 0.0
    assert win == (0, 0) and (blind[0][:3, :3] == blind[0][0, 0]).all() and not blind[2][:3, :3].any()
    assert blind[0][0, 0] - rest.max() >= room * blind[1][0, 0] and blind[0][0, 0] > 10 * plain[0].max()


def test_argument_validation_without_a_device():
    import deconvolve as dv
    from lib import _native, utils
    shape = (40, 50, 3)
    assert _native.IMG_MASK_CELL == mr.CELL
    assert _native.window_scores_args(16, None, 0.99, shape) == (16, (0, 40, 0, 50), float(np.float32(0.99)))
    assert _native.window_scores_args(31, (3, 39, 5, 48), np.inf, shape) == (31, (3, 39, 5, 48), math.inf)
    for bad in (15, 0, -16, 16.5, "16", None, True):
        with pytest.raises(ValueError, match="size"):
            _native.window_scores_args(bad, None, 0.99, shape)
    for region in ((0, 0, 0, 50), (0, 41, 0, 50), (-1, 40, 0, 50), (0, 40, 10, 10), (0, 40), "all", (0.5, 40, 0, 50), (0, 40, 0, 15), (0, 15, 0, 50)):
        with pytest.raises(ValueError, match="region"):
            _native.window_scores_args(16, region, 0.99, shape)
    with pytest.raises(ValueError, match="region"):
        _native.window_scores_args(41, None, 0.99, shape)
    for bad in (0, -1.0, math.nan, "0.99", None, True):
        with pytest.raises(ValueError, match="clip"):
            _native.window_scores_args(16, None, bad, shape)
    pic = np.zeros(shape, np.float32)
    for bad in (15, 1, 0, 20.5, "63", None):
        with pytest.raises(ValueError, match="mask_size"):
            utils.best_mask(pic, bad)
    with pytest.raises(ValueError, match="H x W x 3"):
        utils.best_mask(np.zeros((40, 50)))
    with pytest.raises(ValueError, match="region"):
        utils.best_mask(pic, 63)
    with pytest.raises(ValueError, match="region"):
        utils.best_mask(pic, 17, region=(0, 41, 0, 50))
    with pytest.raises(ValueError, match="clip"):
        utils.best_mask(pic, 17, clip=0.0)
    assert utils.best_mask_args(17, 0.5, None, shape) == (17, (0, 40, 0, 50), 0.5) and utils.best_mask_args(16, 0.5, None, shape)[0] == 17
    assert dv._mask_args(None) is None and dv._mask_args([20, 25]) is None and dv._mask_args((np.int64(20), 25)) is None
    assert dv._mask_args("auto") == 0.99 and dv._mask_args(("auto", 0.5)) == 0.5 and dv._mask_args(["auto", np.inf]) == math.inf
    # deblur_module: refused before anything is uploaded, on both paths
    u8 = np.zeros((40, 50, 3), np.uint8)
    for resident in (True, False):
        for bad in ("automatic", "", ("auto",), ("auto", 0.0), ("auto", -1), ("auto", "x"), ("auto", 0.5, 1), ("best", 0.5), [20], [20, 25, 3], [20.0, 25.0],
                    [20, None], 20, 2.5, (True, False), {"y": 1, "x": 2}):
            with pytest.raises(ValueError, match="mask"):
                dv.deblur_module(u8, "x", ".", 5, mask=bad, save=False, display=False, device_resident=resident)


def test_header_and_export():
    from lib import _native
    header = open(os.path.join(ROOT, "include", "ics_hip.h")).read()
    assert re.search(r"int ics_img_window_scores\(const ics_img \*src, int y0, int y1, int x0, int x1, int size, float clip, int \*box_y, int \*box_x, double \*score, "
                     r"double \*trace,\s+long long \*clipped, double \*map, int map_rows, int map_cols\);", header)
    assert "#define ICS_IMG_MASK_CELL 16" in header and re.search(r"#define ICS_ABI_VERSION 4\b", header)
    lib = _native.load()
    assert lib.ics_abi_version() == _native.ICS_ABI_VERSION == 4
    assert lib.ics_img_window_scores.restype is C.c_int and len(lib.ics_img_window_scores.argtypes) == 15
    assert _native.WindowScores._fields == ("box_y", "box_x", "score", "trace", "clipped", "map")
    assert callable(_native.DeviceImage.window_scores)
