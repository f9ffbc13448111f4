#!/usr/bin/env python3
"""coarse_time_fix (gpsmi.snapshot) under code-phase noise, on the CPU.

    python tools/snapshot_noise.py [--trials 200] [--sigma 0.05]

Truth measurements of the 1-s strong scene of tests/snapshot_truth.py with seeded Gaussian noise of
--sigma samples on every code phase, the a-priori 20 km and 10 s off: fix error (median, worst), how
many fixes were refused, the geometry factor g and protect_m, for all eight satellites, six of them
and five of them."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ('gps-sdr-receiver_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

SETS = [('eight', list(range(8))), ('six', [0, 1, 2, 3, 4, 5]), ('five', [0, 2, 4, 5, 7])]


def main():
    import snapshot_truth as T
    from gpsmi import snapshot as S
    ap = argparse.ArgumentParser()
    ap.add_argument('--trials', type=int, default=200)
    ap.add_argument('--sigma', type=float, default=0.05)
    a = ap.parse_args()
    sc, info = T.strong()
    mid = 1024000
    truth = T.truth_meas(sc, mid)
    rng = np.random.default_rng(79)
    u = np.array([0.6, 0.0, 0.8])
    for name, idx in SETS:
        err, refused, fx = [], 0, None
        for _ in range(a.trials):
            m = truth[idx].copy()
            m['code_phase'] = (m['code_phase'] + rng.normal(0.0, a.sigma, len(m))) % sc.code_samples
            fx = S.coarse_time_fix(m, info['ephs'], T.t_gps_of(info, mid) + 10.0, T.TRUTH + 20.0e3 * u)
            if fx.ok:
                err.append(np.linalg.norm(fx.ecef - T.TRUTH))
            else:
                refused += 1
        print(f"{name} satellites (PRNs {[int(p) for p in truth['prn'][idx]]}), sigma {a.sigma} sample, {a.trials} trials: "
              f"median {np.median(err):.1f} m, worst {np.max(err):.1f} m, refused {refused}; g {fx.g:.2f}, "
              f"protect_m {fx.protect_m:.0f}")


if __name__ == '__main__':
    main()
