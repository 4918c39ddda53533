"""Shapes, contracts and the tolerance against the float64 reference shared by tests/test_basket_greeks_reference.py
(CPU: where the tolerance is measured) and tests/test_gpu_basket_greeks.py (GPU: where it is applied)."""

from __future__ import annotations

import functools

import numpy as np

from spectralmc_amd.basket import BasketConfig
from tests.helpers import basket_reference as br

SEED = 7
ORD0 = 3

# (A, T, P, norm, B): tests/test_gpu_basket_price.py's shapes
CASES = [
    (4, 16, 4096, 1, 12),   # lds, two chunks
    (3, 5, 2048, 1, 12),    # odd A: a discarded normal
    (1, 3, 2048, 0, 12),    # A = 1, RAW
    (8, 2, 2048, 1, 12),    # A = 8: five payoff passes
    (2, 4, 693, 1, 12),     # P % 4 != 0, a partial chunk
    (4, 1, 528, 0, 12),     # T = 1, RAW, a partial chunk
    (2, 3, 65536, 1, 3),    # parked block too large: replay by itself
    (4, 3, 2048, 1, 300),   # more contracts than CUs
]

# (A, T, P, norm, B) of the comparison with the float64 reference: the shapes above on Sobol-drawn contracts
REFERENCE_CASES = [(4, 16, 4096, 1, 6), (3, 5, 2048, 1, 6), (1, 3, 2048, 0, 6), (8, 2, 2048, 1, 6), (2, 4, 693, 1, 6),
                   (4, 1, 528, 0, 6), (2, 3, 65536, 1, 3)]
# every other (A, normalisation), at the smallest shape that still runs the pass plan of its A, the park block and the
# normalisation sweep (one stream per group, a ragged lane, a partial chunk): tests/test_instantiation_ledger.py holds
# the table to the ledger of instantiations, and each row below is the only one of its (A, normalisation)
LEDGER_CASES = [(A, 3, 693, 1, 3) for A in (1, 5, 6, 7)] + [(A, 3, 693, 0, 3) for A in (2, 3, 5, 6, 7, 8)]
REFERENCE_CASES += LEDGER_CASES

# The largest departure of the float32 restatement (portable math, the oracle's kernel-mode terminal values) from the
# float64 reference over REFERENCE_CASES, as a share of the column's own standard error: measured 1.11e-3 (theta call of
# (1, 3, 2048, RAW)) by test_restatement_against_the_reference, which holds the figure below to the measurement.  The
# GPU test allows 4 times that.
MEASURED_SHARE = 1.2e-3
ALLOWED_SHARE = 4 * MEASURED_SHARE


@functools.lru_cache(maxsize=None)
def contracts(A: int, n: int) -> np.ndarray:
    """tests/test_gpu_basket_price.py's generator: [n, 3A + 4] rows K, T, r, rho, X0.., d.., v.."""
    rng = np.random.default_rng(2026 + A)
    rows = []
    for _ in range(n):
        x0 = rng.uniform(50, 150, A)
        k = x0.mean() * rng.uniform(0.8, 1.25)
        t, r, rho = rng.uniform(0.25, 2), rng.uniform(-0.02, 0.08), rng.uniform(-0.1, 0.8)
        d, v = rng.uniform(0, 0.04, A), rng.uniform(0.1, 0.6, A)
        rows.append([k, t, r, rho, *x0, *d, *v])
    out = np.array(rows, dtype=np.float64)
    out.setflags(write=False)
    return out


def sobol_rows(oracle, A: int, n: int, skip: int = 0) -> np.ndarray:
    """tests/test_gpu_basket_reference.py's generator: Sobol points in the default bounds of the basket engine."""
    lo, hi = BasketConfig(n_assets=A, network_size=64, batches_per_mc_run=32).arrays()
    return oracle.sobol_contracts(SEED, skip, n, lo, hi)


def rho_constant_bound(rows: np.ndarray, A: int) -> np.ndarray:
    """[B]: how far the float32 constant crho = df * (f32(T) * K) may lie from T K e^{-r T}: the roundings of T and K, of
    the two products, and df's own bound (basket_reference.forwards).  The rho term of a path is 0 or -+ crho, so the
    column of a contract whose every path is exercised is that constant and its standard error is 0 (rounding noise
    in float64): a share of the standard error alone would ask a float32 constant to be exact."""
    K, Tm, r = rows[:, 0], rows[:, 1], rows[:, 2]
    _, _, df, edf = br.forwards(rows, A)
    return Tm * K * df * br.compose(edf, br.U, br.U, br.U, br.U)


def shares_of_stderr(got: np.ndarray, ref: np.ndarray, rows: np.ndarray, A: int) -> dict[int, float]:
    """Per mean column (the 4A + 6 Greeks and the two prices): the largest |got - ref| over the contracts as a share of
    the reference's standard error of that column; the rho columns first give up rho_constant_bound.  0 / 0 counts as 0,
    anything else over 0 and NaN as inf."""
    n = 4 * A + 6
    const = rho_constant_bound(rows, A)
    out = {}
    for col in list(range(n)) + [2 * n, 2 * n + 1]:
        se = ref[:, col + n if col < n else col + 2]
        err = np.abs(got[:, col] - ref[:, col])
        if col in (4 * A, 4 * A + 1):
            err = np.maximum(err - const, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0.0, 0.0, err / se)
        share = np.where(np.isnan(share), np.inf, share)
        out[col] = float(share.max())
    return out
