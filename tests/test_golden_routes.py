"""Which kernel families the whole-loop reference fixtures reach under ICS_CONV_AUTO (CPU only: ics_describe needs no device).

AUTO's thresholds (csrc/ics_route.hip: the small-frame kernel, fft_preferred) decide which family a fixture exercises when a GPU
test runs it with conv=0.  When they moved in round 6 the fp16-split matrix cores (conv family 1) silently lost most of their
whole-loop coverage.  This pins it: if a threshold moves and a family or a PSF size drops out, the fix is a forced `conv`
parametrisation or a new fixture (oracle/make_golden_levels.py), not lost coverage."""
import glob
import json
import os

import numpy as np
import pytest

from helpers import LEVEL_FIXTURES


def _route(meta):
    from lib import _native as nv
    iters = meta.get("iters", meta.get("snaps", [1]))
    iters = max(iters) if isinstance(iters, list) else iters
    p = nv.RLJob.params(*meta["window"], meta["tau"], iters, meta["step"], meta["lambd"], meta["blind"], correlation=meta.get("corr", 0))
    return nv.describe(meta["M"], meta["N"], meta["MK"], p)


def _whole_loop_fixtures(golden_dir):
    """name -> meta of every fixture holding one reference call's (or chain's) trajectory on one frame"""
    out = {}
    for path in sorted(glob.glob(os.path.join(golden_dir, "rl_*.npz"))):
        meta = json.loads(str(np.load(path)["meta"]))
        if "MK" in meta:                 # rl_black.npz holds many small cases of its own (test_gpu_black.py)
            out[os.path.basename(path)[3:-4]] = meta
    return out


@pytest.mark.parametrize("name", LEVEL_FIXTURES)
def test_level_fixture_runs_on_the_fp16_split_matrix_cores_under_auto(golden_dir, name):
    meta = _whole_loop_fixtures(golden_dir)[name]
    r = _route(meta)
    assert (r.conv_family, r.conv_fp16_split) == (1, 1), (name, r.conv_family, r.conv_fp16_split)


def test_auto_reaches_every_family_with_blind_and_non_blind_fixtures(golden_dir):
    reached = {}
    for name, meta in _whole_loop_fixtures(golden_dir).items():
        r = _route(meta)
        reached.setdefault((r.conv_family, bool(meta["blind"])), []).append((name, meta["MK"]))
    print({k: v for k, v in sorted(reached.items())})
    for fam in (1, 5, 6):
        for blind in (False, True):
            assert (fam, blind) in reached, ("no %s whole-loop fixture reaches conv family %d under AUTO"
                                             % ("blind" if blind else "non-blind", fam), reached)
    ks = {k for _, k in reached[(1, False)]}
    for k in (3, 5, 7):
        assert k in ks, ("no non-blind fixture reaches the matrix cores with a %d x %d PSF" % (k, k), ks)
    assert max(ks) >= 9, ks
