"""bench.py: a plain run measures the headline alone; `--full` adds the secondary measurements after the timed region, without
changing what the timed run computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_full():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "10", "--warmup", "5", "--size", "512", "--psf", "9"] + list(args),
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    for d in (plain, full):
        assert d["steps"] == 10 and d["warmup"] == 5 and d["unit"] == "MPixels/s/iter" and d["higher_is_better"] is True and d["dtype"]
        assert abs(d["value"] - 512 * 512 * 10 / (d["ms_per_step"] * 10 * 1e-3) / 1e6) < 0.01 * d["value"]
        assert d["kernels_ms"] and d["roofline"] is not None
    assert plain["sustained"] is None and plain["other_mode_same_frame"] is None and "cpu_baseline" not in plain
    assert full["sustained"]["steps"] == 200 and full["other_mode_same_frame"]["mode"] == "nonblind"
    # the secondary blocks run after the dump: both runs hand back the same arrays
    for name in ("u", "psf"):
        np.testing.assert_allclose(np.load(tmp_path / "full" / (name + ".npy")), np.load(tmp_path / "plain" / (name + ".npy")), rtol=1e-6, atol=0, err_msg=name)
