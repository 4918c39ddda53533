"""Shapes, inputs and the tolerance against the float64 reference shared by tests/test_basket_general_greeks_reference.py
(CPU: where the tolerance is measured) and tests/test_gpu_basket_general_greeks.py (GPU: where it is applied).

Inputs are tests/helpers/basket_general_cases.py's: Sobol-drawn rows with Dirichlet weights, drawn correlation matrices
and strikes_at_the_forward (drawn_case), and the exchange option on drawn rows (spread_case: weights (1, -1), K = 0)."""

from __future__ import annotations

import functools

import numpy as np

from tests.helpers import basket_general_cases as gcases
from tests.helpers import basket_greeks_cases as eq_cases

SEED, ORD0 = gcases.SEED, gcases.ORD0

# Where A = 8 leaves the lds mode: 8 * roundup4(P) * 4 + 15968 bytes of scratch against 144 KiB
PARK_LAST, PARK_FIRST_REPLAY = 4108, 4109

# (kind, A, T, P, norm, B) of the comparison with the float64 reference: every asset count that takes another pass plan
# (1..3 one pass, 5 and 8 several), odd A (a discarded normal), T in {1, 3, 16}, P one below and one above a chunk, both
# sides of the parking bound at A = 8, RAW and NORMALIZE, and the spread
REFERENCE_CASES = [
    ("drawn", 1, 3, 2047, 0, 3),
    ("drawn", 2, 1, 2049, 1, 4),
    ("drawn", 3, 16, 2047, 1, 3),
    ("drawn", 5, 3, 2049, 1, 3),
    ("drawn", 5, 1, 2047, 0, 3),
    ("drawn", 8, 3, PARK_LAST, 1, 3),
    ("drawn", 8, 1, PARK_FIRST_REPLAY, 1, 3),
    ("spread", 2, 3, 2049, 1, 4),
    ("spread", 2, 3, 2047, 0, 4),
]
# every other (A, normalisation), at the smallest shape that still runs the pass plan and the pair columns of its A, the
# park block and the normalisation sweep (one stream per group, a ragged lane, a partial chunk):
# tests/test_instantiation_ledger.py holds the table to the ledger of instantiations, and each row below is the only one
# of its (A, normalisation)
LEDGER_CASES = ([("drawn", A, 3, 693, 1, 3) for A in (1, 4, 6, 7)]
                + [("drawn", A, 3, 693, 0, 3) for A in (3, 4, 6, 7, 8)])
REFERENCE_CASES += LEDGER_CASES

# The largest departure of the float32 restatement (tests/helpers/basket_general_greeks_restate.py: portable math, a
# float32 walk of the step with the general factor) from the float64 reference over REFERENCE_CASES, as a share of the
# column's own standard error: measured 2.34e-5 (the put price of (1, 3, 2047, RAW)) by
# test_restatement_against_the_reference, which holds the figure below to the measurement.  The GPU test allows 4 times
# that (hw math and the kernel's sum order: DESIGN.md 3.2j's margin).
MEASURED_SHARE = 2.5e-5
ALLOWED_SHARE = 4 * MEASURED_SHARE


@functools.lru_cache(maxsize=None)
def _inputs(kind: str, A: int, B: int):
    import oracle

    oracle.build()
    rows, w, C = gcases.spread_case(oracle, B) if kind == "spread" else gcases.drawn_case(oracle, A, B)
    for a in (rows, w, C):
        a.setflags(write=False)
    return rows, w, C


def inputs(kind: str, A: int, B: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(rows [B, 3A + 4], weights [B, A], correlation [B, A, A]), read-only and shared."""
    return _inputs(kind, A, B)


def greek_columns(A: int) -> int:
    return 4 * A + 4 + A * (A - 1)


def shares_of_stderr(got: np.ndarray, ref: np.ndarray, rows: np.ndarray, A: int) -> dict[int, float]:
    """Per mean column (the n Greeks and the two prices): the largest |got - ref| over the contracts as a share of the
    reference's standard error of that column; the rho columns first give up rho_constant_bound.  0 / 0 counts as 0,
    anything else over 0 and NaN as inf."""
    n = greek_columns(A)
    const = eq_cases.rho_constant_bound(rows, A)
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
