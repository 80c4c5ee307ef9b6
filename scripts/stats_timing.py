"""Device time of one stop-test statistics evaluation (A18 + A19, csrc/ics_stats.hip) per window size, against the outer iteration it
runs beside (GPU box).  Non-blind runs of two outer iterations on smooth synthetic frames with a 3 x 3 PSF, params.profile = 1: the library
brackets every launch group with HIP events on its stream (ics_rl_stats.ms_kernel = average ms per launch of a class).  The first
run of each case is a warm-up (window buffers, LDS configuration).

    python scripts/stats_timing.py [--only NAME ...]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-cases-studies_amd"))
from lib import _native as nv  # noqa: E402

# name, frame M x N, stats window (top, bottom, left, right)
CASES = [
    ("1024^2", 1100, 1100, (38, 1062, 38, 1062)),          # P x P path, P = 2048
    ("4096^2", 4100, 4100, (2, 4098, 2, 4098)),            # P x P path, P = 8192
    ("4200^2", 4210, 4210, (5, 4205, 5, 4205)),            # long-line path, 16384 x 16384
    ("8300x200", 8310, 220, (5, 8305, 10, 210)),           # long-line path, 32768 x 512
    ("13000^2 whole frame", 13000, 13000, (0, 13000, 0, 13000)),   # long-line path, 32768 x 32768
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    MK, outer = 3, 2
    rng = np.random.default_rng(0)
    for name, M, N, win in CASES:
        if args.only and name not in args.only:
            continue
        pad = MK // 2
        job = nv.RLJob(M, N, MK)
        try:
            # a smooth picture plus a little noise: a well-posed problem (a uniformly random image with this PSF diverges to NaN)
            yy = np.sin(np.linspace(0, 7, M, dtype=np.float32))[:, None, None]
            xx = np.cos(np.linspace(0, 5, N, dtype=np.float32))[None, :, None]
            image = (0.5 + 0.2 * yy * xx + 0.01 * rng.standard_normal((M, N, 3), dtype=np.float32)).astype(np.float32)
            u = np.pad(image, ((pad, pad), (pad, pad), (0, 0)), mode="edge")
            job.upload(image, u, np.full((MK, MK, 3), 1.0 / (MK * MK), np.float32))
            p = job.params(*win, 1e9, outer, 1e-3, 10000.0, False, profile=1)
            job.run(p)
            job.upload(image, u, np.full((MK, MK, 3), 1.0 / (MK * MK), np.float32))
            st = job.run(p)
            k = nv.KERNEL_NAMES.index("stats")
            stats_ms = float(st.ms_kernel[k])
            outer_ms = float(st.ms_total) / max(1, st.iterations_done)
            print(json.dumps({"window": name, "H": win[1] - win[0], "W": win[3] - win[2], "frame": [M, N],
                              "stats_ms": round(stats_ms, 4), "stats_launches": int(st.launches[k]),
                              "outer_iteration_ms": round(outer_ms, 4), "stats_share_of_outer": round(stats_ms / outer_ms, 3),
                              "M_r": float(st.M_r)}), flush=True)
        finally:
            job.close()


if __name__ == "__main__":
    main()
