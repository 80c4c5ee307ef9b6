"""CPU: the skip rule of csrc/ics_maxg_select.h -- which tiles k_maxg_select may leave unread behind the operand-free mode-2 launch -- run by the
stand-alone host program csrc/tools/check_maxg_skip.hip on random and adversarial float32 frames (denormals, values one ulp apart, overflowing
and underflowing lambd, zeros, NaN, inf).  The program checks with the header's own functions that no pixel of a skipped tile exceeds the
rule's lower bound, that the tile holding max |gradu| is never skipped, and that the key of max |g| over the scanned tiles equals the key over
all tiles in every bit (exit status).  Nothing is loaded into Python.  What the kernels make of the rule: tests/test_gpu_maxg_select.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-cases-studies_amd", "csrc")


@pytest.fixture(scope="module")
def tool():
    assert shutil.which("make"), "no make"
    subprocess.check_call(["make", "-C", CSRC, "tools/check_maxg_skip"], stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "tools", "check_maxg_skip")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_no_skipped_tile_can_hold_the_maximum(tool, seed):
    r = subprocess.run([tool, "300000", str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "the skip rule is violated, or the tool failed: %s" % r.stderr
    assert "no violation" in r.stdout and " 0 tiles skipped" not in r.stdout, r.stdout      # (the rule does skip: the check is not vacuous)
