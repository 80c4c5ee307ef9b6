"""CPU: the PSF step A14-A17 as csrc/ics_psf_step.h states it -- the functions k_psf_spectra calls in every workgroup -- run by the
stand-alone host program csrc/tools/check_psf_step.hip.  The program itself compares the header's functions bit for bit with its own
float32 restatement of lib/deconvolution.pyx:574-589 (exit status); here its output is held against the oracle's step
(helpers.psf_step_f32: numpy float32 + rl_mm_oracle.normalize_kernel) at the gate of the whole-call PSF comparisons of
tests/test_gpu_rl.py.  Nothing is loaded into Python.  What the kernels make of the same functions: tests/test_gpu_psf_step_tiles.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rl_mm_oracle as orc
from helpers import psf_step_f32, rel_err
from test_gpu_rl import TRAJ_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-cases-studies_amd", "csrc")


@pytest.fixture(scope="module")
def tool():
    assert shutil.which("make"), "no make"
    subprocess.check_call(["make", "-C", CSRC, "tools/check_psf_step"], stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "tools", "check_psf_step")


def _inputs(MK, seed):
    """a per-channel PSF without symmetry and a gradient of both signs; with step = MK / 2 the largest decrement is half the PSF's
    maximum, so the faint taps go negative and the clamp is live"""
    rng = np.random.default_rng(seed)
    psf = (orc.gaussian_psf(MK) * (0.5 + rng.random((MK, MK, 3), dtype=np.float32))).astype(np.float32)
    orc.normalize_kernel(psf, MK)
    gradk = (rng.standard_normal((MK, MK, 3)) * 37.0).astype(np.float32)
    return psf, gradk


def _run(tool, tmp_path, psf, gradk, step, correlation):
    MK = psf.shape[0]
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    with open(src, "wb") as f:
        f.write(np.array([MK, int(correlation)], np.int32).tobytes())
        f.write(np.array([step], np.float32).tobytes())
        f.write(np.ascontiguousarray(psf, np.float32).tobytes())
        f.write(np.ascontiguousarray(gradk, np.float32).tobytes())
    r = subprocess.run([tool, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, "header and restatement differ, or the tool failed: %s" % r.stderr
    raw = np.fromfile(dst, np.float32)
    n = psf.size
    assert raw.size == 2 * n + 1
    return raw[:n].reshape(psf.shape), raw[n:2 * n].reshape(psf.shape), raw[2 * n]


@pytest.mark.parametrize("correlation", [0, 1], ids=["percolour", "correlation"])
@pytest.mark.parametrize("MK", [3, 15, 25, 45])
def test_header_step_equals_restatement_and_oracle(tool, tmp_path, MK, correlation):
    psf, gradk = _inputs(MK, seed=MK)
    step = MK / 2.0
    local, caller, dtpsf = _run(tool, tmp_path, psf, gradk, step, correlation)
    want_local, want_caller, want_dt = psf_step_f32(psf, gradk, step, MK, correlation)
    stepped = psf - want_dt * gradk
    assert (stepped < 0).sum() >= 2, "the clamp is not live"
    e_local, e_caller = rel_err(local, want_local), rel_err(caller, want_caller)
    print("K=%d correlation=%d: dtpsf %.9g / %.9g, rel err local %.2e caller %.2e (gate %.0e), %d taps clamped" % (
        MK, correlation, dtpsf, want_dt, e_local, e_caller, TRAJ_TOL, int((stepped < 0).sum())))
    assert abs(float(dtpsf) - float(want_dt)) <= TRAJ_TOL * abs(float(want_dt))
    assert e_local < TRAJ_TOL and e_caller < TRAJ_TOL
    assert (local >= 0).all()
    if correlation:
        assert np.array_equal(local[..., 0], local[..., 1]) and np.array_equal(local[..., 0], local[..., 2])
        assert (caller < 0).any()       # the caller's array keeps the raw step (pyx:585 rebinds the name)
    else:
        assert np.array_equal(local, caller)


def test_step_without_a_live_clamp(tool, tmp_path):
    """the shipped step size: no tap changes sign, the same comparisons"""
    psf, gradk = _inputs(15, seed=2)
    local, caller, dtpsf = _run(tool, tmp_path, psf, gradk, 1e-3, 0)
    want_local, want_caller, want_dt = psf_step_f32(psf, gradk, 1e-3, 15, 0)
    assert ((psf - want_dt * gradk) >= 0).all()
    assert rel_err(local, want_local) < TRAJ_TOL and rel_err(caller, want_caller) < TRAJ_TOL
