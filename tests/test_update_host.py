"""CPU: the image update A5-A10 as csrc/ics_update.h states it -- the functions every update kernel calls -- run value by value by the
stand-alone host program csrc/tools/check_update_px.hip and compared bit for bit with the numpy float32 restatement
(helpers.update_f32).  Nothing is loaded into Python.  What the kernels make of the same functions: tests/test_gpu_black.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rl_mm_oracle as orc
from helpers import update_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-cases-studies_amd", "csrc")
STEP, LAMBD = 1e-3, 10000.0


@pytest.fixture(scope="module")
def tool():
    assert shutil.which("make"), "no make"
    subprocess.check_call(["make", "-C", CSRC, "tools/check_update_px"], stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "tools", "check_update_px")


def _key(f):
    """ics_f2key (csrc/ics_common.h)"""
    b = int(np.float32(f).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def _with_gradient(image, u0, pad, seed):
    """u, ut and a back-projection for a frame: the back-projection is exactly 0 wherever the image is (0/0 pixels), one of those
    zeros is -0.0, and so is one value of u"""
    rng = np.random.default_rng(seed)
    M, N = image.shape[:2]
    ut = u0
    u = (ut + 0.02 * rng.standard_normal(ut.shape)).astype(np.float32)
    u[ut == 0] = 0.0
    g = (1e-5 * rng.standard_normal(ut.shape)).astype(np.float32)
    gi = g[pad:pad + M, pad:pad + N]
    gi[image == 0] = 0.0
    zy, zx, zc = np.argwhere(image == 0)[3]
    gi[zy, zx, zc] = -0.0
    u[pad + zy, pad + zx, (zc + 1) % 3] = -0.0
    assert ((gi == 0) & (image == 0)).sum() > 10
    return u, ut, g


def _frame_small():
    """13 x 11 with pad 2: a row of 3 * 15 = 45 floats, no multiple of 4"""
    rng = np.random.default_rng(7)
    M, N, pad = 13, 11, 2
    image = (0.1 + 0.8 * rng.random((M, N, 3))).astype(np.float32)
    image[4:8] = 0.0
    u0 = np.ascontiguousarray(np.pad(image, ((pad, pad), (pad, pad), (0, 0)), mode="edge"))
    return image, u0, pad


def _frame_band():
    case = orc.black_case(41, 53, 5, "band_mid", seed=5)
    return case["image"], case["u0"], 2


FRAMES = {"13x11": _frame_small, "41x53_band": _frame_band}


def _run(tool, tmp_path, image, u, ut, g, blind, pad):
    M, N = image.shape[:2]
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    with open(src, "wb") as f:
        f.write(np.array([M, N, pad, int(blind)], np.int32).tobytes())
        f.write(np.array([STEP, LAMBD], np.float32).tobytes())
        for a in (u, ut, g, image):
            f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    r = subprocess.run([tool, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(dst, np.uint32)
    assert raw.size == u.size + 6
    return raw[:u.size].view(np.float32).reshape(u.shape), raw[u.size:u.size + 3].view(np.float32), raw[u.size + 3:]


@pytest.mark.parametrize("blind", [False, True], ids=["nonblind", "blind"])
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_header_update_equals_the_numpy_restatement(tool, tmp_path, frame, blind):
    image, u0, pad = FRAMES[frame]()
    u, ut, g = _with_gradient(image, u0, pad, seed=1)
    got, dt, keys = _run(tool, tmp_path, image, u, ut, g, blind, pad)
    want, dt_want, DoF = update_f32(u, ut, g, image, STEP, LAMBD, blind, pad)
    assert not np.isnan(want).any()
    assert np.array_equal(got, want)
    assert np.array_equal(dt, dt_want)
    assert int(keys[0]) == _key(DoF.min()) and int(keys[1]) == _key(DoF.max()) and int(keys[2]) == 0


def test_a_nan_in_the_back_projection_raises_the_flag(tool, tmp_path):
    image, u0, pad = _frame_small()
    u, ut, g = _with_gradient(image, u0, pad, seed=2)
    g[pad + 1, pad + 2, 1] = np.nan
    _, _, keys = _run(tool, tmp_path, image, u, ut, g, False, pad)
    assert int(keys[2]) == 1
