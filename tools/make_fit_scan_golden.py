"""Generate tests/golden/fit_scan_trajectory.npz: the float64 ICP loop of tests/closest_ref.py (icp_oracle) on the inputs of
closest_ref.scan_case() -- from zero, lr 0.05, 300 iterations, closest points at every iteration -- and the same loop in float32 for
100 iterations.  The file holds data only: the float64 parameters after 20, 100 and 300 iterations, the float32 loop's worst
parameter difference to them after 20 and 100 (the yardstick of tests/test_gpu_morphable_fit_scan.py), the model-to-scan surface
RMS at the start and at the end, and the first 20 losses.  tests/test_closest_cpu.py recomputes the float64 loop and compares; the
GPU tests read the file, so that they do not spend a minute of numpy on it.

    python tools/make_fit_scan_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import closest_ref as R  # noqa: E402


def main():
    m, p_true, scans = R.scan_case()
    o64 = R.icp_oracle(m, scans, iters=300, lr=0.05, keep=(20, 100))
    o32 = R.icp_oracle(m, scans, iters=100, lr=0.05, keep=(20, 100), dtype=np.float32)
    first, last = R.surface_rms(m, np.zeros_like(p_true), scans), R.surface_rms(m, o64["p"], scans)
    yard = {k: np.abs(o32["snapshots"][k].astype(np.float64) - o64["snapshots"][k]).max() for k in (20, 100)}
    print(f"surface RMS {first} -> {last} (ratio {last / first}); float32 loop differs by {yard}")
    np.savez(os.path.join(ROOT, "tests", "golden", "fit_scan_trajectory.npz"), p20=o64["snapshots"][20], p100=o64["snapshots"][100],
             p300=o64["p"], yard20=yard[20], yard100=yard[100], rms_first=first, rms_last=last, loss20=o64["loss_history"][:20])


if __name__ == "__main__":
    main()
