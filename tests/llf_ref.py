"""Fast local Laplacian filter (Paris, Hasinoff, Kautz 2011, in the sampled form of Aubry et al. 2014) in numpy: the specification
of ics_img_local_laplacian / DeviceImage.local_laplacian (csrc/ics_img_llf.hip) with the dtype as a parameter: float64 is the oracle
of the tests, float32 the restatement whose distance from the oracle sets their gates.  The restatement performs the kernel's
operations in the kernel's order (llf_signal / llf_remap / llf_reduce5 / llf_expand1 / llf_blend there), every product and sum rounded
on its own: no FMA.

    signal   "channel": each channel by itself, out_c = R[0] of that channel;
             "vector":  Y = (0.2126 R + 0.7152 G) + 0.0722 B, out_c = in_c + (Y' - Y), Y' = R[0]
    reduce   size n -> (n + 1) // 2: taps 1 4 6 4 1 at the input indices 2 y - 2 .. 2 y + 2, folded by the symmetric extension
             (numpy.pad(mode="symmetric"), at any distance), (((a0 + a4) + 2 a2) + 4 a2) + 4 (a1 + a3) along y, then the same along
             x, then times 1 / 256.  (The weight 6 is split into 2 + 4 so that every partial sum of a constant c is c times a power of
             two, 2 c, 4 c, 8 c, 16 c: a constant is reduced to itself exactly whatever its bits.  ((a0 + a4) + 4 (a1 + a3)) + 6 a2
             rounds 10 c and 6 c.)
    expand   to a given size, indices clamped to the coarse level: position 2 k: (((c[k-1] + c[k+1]) + 2 c[k]) + 4 c[k]) 0.125 (the same split
             of the 6), position 2 k + 1: (c[k] + c[k+1]) 0.5; along y, then along x
    remap    about g, d = i - g:  r_g(i) = g + d (edges + (detail - edges) exp((d d) ninv)),  ninv = float32(-1 / (2 sigma^2))
    samples  g_k = k / (K - 1), k = 0 .. K - 1
    pyramids G[0..J] of the signal, P_k[0..J] of r_{g_k}(signal), L_k[l] = P_k[l] - expand(P_k[l+1])
    output Laplacian at level l < J, pixel p:  t = clamp(G[l](p) (K - 1), 0, K - 1), k0 = min(floor(t), K - 2), f = t - k0,
             OL[l](p) = a + f (b - a), a = L_k0[l](p), b = L_{k0+1}[l](p)
    collapse R[J] = G[J], R[l] = OL[l] + expand(R[l+1]); the filtered signal is R[0]

`exact` is the unsampled filter for tiny pictures: the coefficient at (l, p) comes from the pyramid of the signal remapped about
g = G[l](p) itself."""
import numpy as np

COUPLINGS = ("channel", "vector")
MAX_LEVELS = 10
MAX_SAMPLES = 16
LUMA = (0.2126, 0.7152, 0.0722)


def symm(i, n):
    """index of the symmetric extension ... x1 x0 | x0 x1 ... x(n-1) | x(n-1) ..., at any distance"""
    i = np.mod(i, 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def default_levels(H, W):
    """the number of halvings that bring the longer side to 16 or below, within 1 .. MAX_LEVELS"""
    n, J = max(int(H), int(W)), 0
    while n > 16:
        n, J = (n + 1) // 2, J + 1
    return min(max(J, 1), MAX_LEVELS)


def _reduce_axis(x, axis):
    n = x.shape[axis]
    m = (n + 1) // 2
    a = [np.take(x, symm(2 * np.arange(m) - 2 + t, n), axis=axis) for t in range(5)]
    two, four = x.dtype.type(2), x.dtype.type(4)
    return (((a[0] + a[4]) + two * a[2]) + four * a[2]) + four * (a[1] + a[3])


def reduce(x):
    """one level down: (n + 1) // 2 per axis, in x.dtype"""
    return _reduce_axis(_reduce_axis(x, 0), 1) * x.dtype.type(1.0 / 256.0)


def _expand_axis(c, n, axis):
    m = c.shape[axis]
    pos = np.arange(n)
    k = pos // 2
    cm, c0, cp = (np.take(c, np.clip(k + d, 0, m - 1), axis=axis) for d in (-1, 0, 1))
    two, four, eighth, half = c.dtype.type(2), c.dtype.type(4), c.dtype.type(0.125), c.dtype.type(0.5)
    even = (((cm + cp) + two * c0) + four * c0) * eighth
    odd = (c0 + cp) * half
    shape = [1, 1]
    shape[axis] = n
    return np.where((pos % 2 == 0).reshape(shape), even, odd)


def expand(c, shape):
    """one level up to `shape`, in c.dtype"""
    return _expand_axis(_expand_axis(c, shape[0], 0), shape[1], 1)


def gaussian_pyramid(x, J):
    pyr = [x]
    for _ in range(J):
        pyr.append(reduce(pyr[-1]))
    return pyr


def laplacian_pyramid(x, J):
    """[L[0] .. L[J-1], G[J]]"""
    g = gaussian_pyramid(x, J)
    return [g[l] - expand(g[l + 1], g[l].shape) for l in range(J)] + [g[J]]


def collapse(lap):
    r = lap[-1]
    for l in range(len(lap) - 2, -1, -1):
        r = lap[l] + expand(r, lap[l].shape)
    return r


def params(sigma, detail, edges, dtype):
    """(ninv, detail - edges, edges) as the device holds them: float32 arguments, the exponent's factor rounded once from float64"""
    s, d, e = np.float32(sigma), np.float32(detail), np.float32(edges)
    ninv = np.float32(-1.0 / (2.0 * float(s) * float(s)))
    return dtype(ninv), dtype(d) - dtype(e), dtype(e)


def remap(i, g, par):
    ninv, de, edges = par
    d = i - g
    return g + d * (edges + de * np.exp((d * d) * ninv))


def sample(k, K, dtype):
    return dtype(k) / dtype(K - 1)


def filter_plane(S, sigma, detail, edges, J, K, dtype=np.float64):
    """the sampled filter of one H x W plane"""
    S = np.asarray(S, dtype=dtype)
    par = params(sigma, detail, edges, dtype)
    G = gaussian_pyramid(S, J)
    L = [laplacian_pyramid(remap(S, sample(k, K, dtype), par), J) for k in range(K)]
    R = G[J]
    for l in range(J - 1, -1, -1):
        t = np.clip(G[l] * dtype(K - 1), dtype(0), dtype(K - 1))
        k0 = np.minimum(np.floor(t), K - 2).astype(np.int64)
        f = t - k0.astype(dtype)
        stack = np.stack([L[k][l] for k in range(K)])
        a = np.take_along_axis(stack, k0[None], axis=0)[0]
        b = np.take_along_axis(stack, k0[None] + 1, axis=0)[0]
        R = (a + f * (b - a)) + expand(R, G[l].shape)
        assert R.dtype == dtype
    return R


def exact_plane(S, sigma, detail, edges, J):
    """the unsampled filter of one tiny plane, float64: a pyramid per coefficient"""
    S = np.asarray(S, dtype=np.float64)
    par = params(sigma, detail, edges, np.float64)
    G = gaussian_pyramid(S, J)
    R = G[J]
    for l in range(J - 1, -1, -1):
        OL = np.empty_like(G[l])
        for p in np.ndindex(*G[l].shape):
            OL[p] = laplacian_pyramid(remap(S, G[l][p], par), J)[l][p]
        R = OL + expand(R, G[l].shape)
    return R


def luma(I):
    w = [I.dtype.type(np.float32(v)) for v in LUMA]
    return (w[0] * I[..., 0] + w[1] * I[..., 1]) + w[2] * I[..., 2]


def _apply(I, coupling, dtype, plane):
    if coupling not in COUPLINGS:
        raise ValueError("coupling %r" % (coupling,))
    I = np.asarray(I, dtype=dtype)
    if coupling == "channel":
        out = np.stack([plane(I[..., c]) for c in range(3)], axis=2)
    else:
        Y = luma(I)
        out = I + (plane(Y) - Y)[..., None]
    assert out.dtype == dtype
    return out


def local_laplacian(I, sigma, detail, edges=1.0, levels=None, samples=8, coupling="vector", dtype=np.float64):
    """I: H x W x 3.  Every operation is carried out in `dtype`."""
    J = default_levels(I.shape[0], I.shape[1]) if levels is None else int(levels)
    K = int(samples)
    if not 1 <= J <= MAX_LEVELS or not K >= 2:
        raise ValueError("levels %r, samples %r" % (levels, samples))
    return _apply(I, coupling, dtype, lambda S: filter_plane(S, sigma, detail, edges, J, K, dtype))


def exact(I, sigma, detail, edges, levels, coupling="vector"):
    return _apply(I, coupling, np.float64, lambda S: exact_plane(S, sigma, detail, edges, int(levels)))
