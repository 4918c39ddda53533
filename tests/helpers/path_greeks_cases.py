"""The inputs of the bound tests of smc_gbm_greeks_paths (tests/test_path_greeks_reference.py on the CPU,
tests/test_gpu_path_greeks_reference.py on the GPU): contract rows near the money with v sqrt(T) >= 0.1, so that few
rows of a path lie within rounding of its extreme (a plain numpy estimate: with a relative row bound of 2e-5 the
near-tie share at 16 rows is about 7e-4 at v sqrt(T) = 0.2 and about 5e-3 at 0.025), and shapes with an odd row count
and a ragged path count, and with two whole chunks.  The CPU test asserts that the reference alone meets both caps on
these inputs.  The flat row (v = 0, r = d: every row equals X0) is held on its delta and rho columns only."""

from __future__ import annotations

import numpy as np

SEED = 7
ORD0 = 11
# X0, K, T, r, d, v
ROWS = np.array([
    [100.0, 100.0, 1.0, 0.03, 0.01, 0.2],
    [100.0, 105.0, 0.5, 0.05, 0.0, 0.3],
    [57.0, 55.0, 2.0, -0.01, 0.02, 0.15],
    [143.0, 150.0, 0.25, 0.08, 0.04, 0.6],
    [0.9, 0.85, 1.5, 0.02, 0.0, 0.45],
    [1000.0, 1010.0, 0.75, 0.04, 0.01, 0.12],
], dtype=np.float64)
ROWS.setflags(write=False)
FLAT_ROWS = np.array([[100.0, 95.0, 2.0, 0.03, 0.03, 0.0]], dtype=np.float64)
FLAT_ROWS.setflags(write=False)
CASES = [(5, 693), (16, 4096)]
assert np.all(ROWS[:, 5] * np.sqrt(ROWS[:, 2]) >= 0.1)
