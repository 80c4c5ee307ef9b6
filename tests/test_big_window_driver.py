"""deconvolve.deblur_module with a stop-test window above 1024 px (no GPU: the solver is a recorder).  The reference takes any
`mask_size` the picture holds (deconvolve.py:138-141); the driver passes the window on to the solver as the reference's arithmetic
gives it, and the library evaluates the stop test on windows of any size a job can hold (ics_stats.hip, long-line path)."""
import numpy as np


def test_mask_size_above_1025_reaches_the_solver_with_the_reference_window(monkeypatch):
    import deconvolve as dv
    import rl_mm_oracle as orc
    monkeypatch.setattr(dv.dc, "normalize_kernel", orc.normalize_kernel)   # no GPU in this test: oracle as stand-in
    calls = []

    def solver(image, u, psf, top, bottom, left, right, tau, M, N, C, MK, iterations, step, lambd, **kw):
        calls.append(dict(win=(top, bottom, left, right), M=M, N=N, MK=MK, blind=kw["blind"], image=image.shape))
        pad = (u.shape[0] - M) // 2
        return u[pad:pad + M, pad:pad + N]

    rng = np.random.default_rng(1)
    pic = (rng.random((1600, 1700, 3)) * 255).astype(np.uint8)
    K, mask_size = 5, 1501
    out, psf = dv.deblur_module(pic, "x", ".", K, mask_size=mask_size, pyramid=False, display=False, save=False, solver=solver,
                                iterations=3)
    assert len(calls) == 2
    # pad_image (1, 1): 1602 x 1702, centre [801, 851]; the box is centre +- mask_size // 2 (deconvolve.py:138-141)
    top, bottom, left, right = 801 - 750, 801 + 750, 851 - 750, 851 + 750
    tt, tb, tl, tr = dv.mask_window(1.0, top, bottom, left, right)
    pad = K // 2
    win = (pad + 1, tb - tt - pad - 1, pad + 1, tb - tt - pad - 1)
    blind, full = calls
    assert blind["blind"] is True and full["blind"] is False
    assert blind["win"] == win and full["win"] == win
    assert win[1] - win[0] > 1024                                       # a window the 1025 cap used to refuse
    assert blind["M"] == tb - tt + 2 and blind["N"] == tr - tl + 2 and blind["MK"] == K
    assert full["image"] == (1603 + 2, 1703 + 2, 3) and full["M"] == 1605 and full["N"] == 1705
    assert out.shape == (1600, 1700, 3)
