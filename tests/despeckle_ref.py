"""Despeckle (thresholded median) in numpy, the specification of ics_img_despeckle / DeviceImage.despeckle
(csrc/ics_img_despeckle.hip).  The result is a selection among the input's values and the decision one correctly rounded float32
subtraction, so the device must give these bits; there is no second precision.

    key      of a float32 with bits b: b ^ 0xFFFFFFFF if the sign bit is set, else b | 0x80000000: unsigned integers in the order of
             the values, -0 below +0, NaNs at the two ends by sign
    window   of (y, x): the (2 r + 1)^2 pixels at (clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)) (np.pad(mode="edge")), n = 9 or 25
    med_c    the value whose key has rank (n - 1) // 2 among the keys of channel c of the window
    d_c      = |I_c - med_c| in float32; hit_c = ~(d_c <= t_c): a NaN difference is a hit
    channel  out_c = med_c where hit_c, else I_c; counts[c] = the hits of channel c
    vector   one threshold; hit = hit_0 | hit_1 | hit_2; all three channels of a hit pixel become their medians; counts[0] = hit pixels
"""
import numpy as np

COUPLINGS = ("channel", "vector")
MAX_RADIUS = 2
STRENGTH = 6.0


def keys(f):
    """the monotone integer keys of float32 values"""
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), b ^ np.uint32(0xFFFFFFFF), b | np.uint32(0x80000000)).astype(np.uint32)


def values(k):
    """the float32 values of keys"""
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(np.float32)


def median(f, radius):
    """the key-order median of the (2 radius + 1)^2 window of every value of an H x W x 3 picture, float32"""
    if radius not in range(1, MAX_RADIUS + 1):
        raise ValueError("radius %r" % (radius,))
    k = keys(f)
    if k.ndim != 3 or k.shape[2] != 3:
        raise ValueError("shape %s" % (k.shape,))
    H, W, r = k.shape[0], k.shape[1], radius
    p = np.pad(k, ((r, r), (r, r), (0, 0)), mode="edge")
    stack = np.stack([p[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)])
    stack.sort(axis=0)
    return values(stack[(stack.shape[0] - 1) // 2])


def despeckle(f, threshold, radius, coupling):
    """(out, counts): out float32 H x W x 3; counts a tuple of three ints ("channel") or of one ("vector").  threshold: one value or
    ("channel") three, taken as float32"""
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    I = np.ascontiguousarray(f, dtype=np.float32)
    med = median(I, radius)
    t = np.broadcast_to(np.asarray(threshold, dtype=np.float32), (3,) if coupling == "channel" else ())
    with np.errstate(invalid="ignore"):
        d = np.abs(I - med)
        assert d.dtype == np.float32
        hit = ~(d <= t)
    if coupling == "vector":
        hit = np.broadcast_to(hit.any(axis=2, keepdims=True), hit.shape)
        counts = (int(hit[..., 0].sum()),)
    else:
        counts = tuple(int(hit[..., c].sum()) for c in range(3))
    out = np.where(hit, med.view(np.uint32), I.view(np.uint32)).astype(np.uint32).view(np.float32)
    return out, counts
