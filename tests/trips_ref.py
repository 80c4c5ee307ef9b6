"""The loop arithmetic of the device-image kernels whose production form only shows past a count: how many units a frame gives a
kernel, how many workgroups its launcher starts for them, and which loop form a lane then runs.  The constants are read from the
sources (csrc/ics_img_*.hip), the launchers' grid rules are restated here; tests/test_trip_counts.py holds the shapes of the GPU tests
to their conditions at 256 CUs, the GPU tests assert the same on the device they run on.

  align reduce  one workgroup of ALRED lanes; parts = ALRED // ns lanes per slot entry, lane (p, k) takes eight tiles a trip while
                t + 7 parts < tiles, then one at a time.  ns = n (n + 1) / 2 + n + 2 for n parameters.
  mask pick     one workgroup of MKPICK lanes; eight candidates a trip while c + 7 MKPICK < cand, then one at a time.
  edge mask     persistent workgroups, at most cus x k: k = 1 ("channel") or 4 ("vector") for the count passes, 8 for the mask kernels;
                units: 4 x 64 pixel tiles (route 1, the keys pass), EDLANES EDHK keys (the later passes of route 2), EDLANES keys (its mask).
  noise         persistent workgroups, at most cus x k: route 1 k = 3 / 4 over 4 x 64 tiles; route 2 k = 2 / 4 over NSTH x NSTW tiles, then
                k = 4 over NSLANES NSHK keys.
  gamma, upload grids of at most GRID_CAP blocks of 256 lanes: a lane takes a second value above 256 GRID_CAP values."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-cases-studies_amd", "csrc")
CUS = 256                       # what csrc/ics_route.hip assumes without a device: an MI355X


def source(unit):
    with open(os.path.join(CSRC, unit)) as fh:
        return fh.read()


def defines(unit, *names):
    """the integer #defines `names` of a unit; ICS_IMG_* values are taken from include/ics_hip.h"""
    src = source(unit)
    header = source(os.path.join("..", "..", "include", "ics_hip.h"))
    out = []
    for name in names:
        m = re.search(r"^#define %s (\w+)\b" % name, src, re.M)
        assert m, (unit, name)
        v = m.group(1)
        if not v.isdigit():
            m = re.search(r"^#define %s (\d+)\b" % v, header, re.M)
            assert m, (unit, name, v)
            v = m.group(1)
        out.append(int(v))
    return out[0] if len(out) == 1 else tuple(out)


def grid_cap():
    """the block cap of grid_for (csrc/ics_img.hip): (cap, lanes per block)"""
    m = re.search(r"inline unsigned grid_for\(long n\) \{ long b = \(n \+ 255\) / 256; return \(unsigned\)\(b > (\d+) \? (\d+) :", source("ics_img.hip"))
    assert m and m.group(1) == m.group(2), "grid_for has changed: restate it here"
    return int(m.group(1)), 256


def ceil_div(a, b):
    return -(-a // b)


# ---- align reduce and mask pick: one workgroup, eight a trip ------------------------------------------------------------------------------
def align_slot_floats(n):
    """ns of a variant with n parameters: the upper triangle of S, g, sum r^2, the count"""
    return n * (n + 1) // 2 + n + 2


def align_tiles(H, W):
    t = defines("ics_img_align.hip", "ALT")
    return ceil_div(H, t) * ceil_div(W, t)


def eight_wide(items, stride):
    """per lane class of a loop `for (; c + 7 stride < items; c += 8 stride) ...; for (; c < items; c += stride) ...` started at
    c = lane < stride: {(unrolled trips, tail steps): number of lanes}"""
    out = {}
    for lane in range(stride):
        c, trips, tail = lane, 0, 0
        while c + 7 * stride < items:
            c, trips = c + 8 * stride, trips + 1
        while c < items:
            c, tail = c + stride, tail + 1
        out[trips, tail] = out.get((trips, tail), 0) + 1
    return out


def align_reduce_forms(H, W, n):
    """eight_wide of k_img_al_reduce for a plane of H x W and n parameters"""
    return eight_wide(align_tiles(H, W), defines("ics_img_align.hip", "ALRED") // align_slot_floats(n))


def pick_forms(cand):
    return eight_wide(cand, defines("ics_img_mask.hip", "MKPICK"))


# ---- persistent workgroups: (units, cap) per kernel ------------------------------------------------------------------------------------------
def edge_mask_grids(H, W, coupling, route, cus=CUS):
    """{kernel: (units, cap)} of ics_launch_img_edge_mask"""
    lanes, hk = defines("ics_img_edges.hip", "EDLANES", "EDHK")
    per_cu = 4 if coupling == "vector" else 1
    tiles, n = ceil_div(W, 64) * ceil_div(H, 4), H * W
    if route == 1:
        return {"k_img_ed_recompute": (tiles, cus * per_cu), "k_img_ed_mask": (tiles, cus * 8)}
    return {"k_img_ed_keys": (tiles, cus * per_cu), "k_img_ed_hist": (ceil_div(n, lanes * hk), cus * per_cu), "k_img_ed_mask_keys": (ceil_div(n, lanes), cus * 8)}


def noise_grids(H, W, coupling, route, cus=CUS):
    """{kernel: (units, cap)} of ics_launch_img_noise"""
    lanes, hk, tw, th = defines("ics_img_noise.hip", "NSLANES", "NSHK", "NSTW", "NSTH")
    vec = coupling == "vector"
    if route == 1:
        return {"k_img_ns_recompute": (ceil_div(W, 64) * ceil_div(H, 4), cus * (4 if vec else 3))}
    return {"k_img_ns_keys": (ceil_div(W, tw) * ceil_div(H, th), cus * (4 if vec else 2)), "k_img_ns_hist": (ceil_div(H * W, lanes * hk), cus * 4)}


def past_the_caps(cus=CUS):
    """(H, W) of a frame on which every persistent kernel of the edge mask and of the noise estimate has more units than workgroups, in
    both couplings: 1030 x 1100 at 256 CUs, its area growing with the CUs.  H is no multiple of 4 or 16, W none of 64."""
    s = (cus / 256.0) ** 0.5
    H, W = int(-(-1030 * s // 1)), int(-(-1100 * s // 1))
    while H % 4 == 0 or H % 16 == 0:
        H += 1
    while W % 64 == 0:
        W += 1
    return H, W


BIG = past_the_caps()           # the frame of the CPU measurements and, on an MI355X, of the GPU tests: (1030, 1100)
STRIDE_FRAME = (2368, 2368)     # x 3 values: past one step of gamma's and the integer upload's grid-stride loops
