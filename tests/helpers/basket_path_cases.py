"""The shapes, contracts and barriers the tests of smc_basket_price_paths share (numpy only), so that the CPU tests of
the reference and the GPU tests of the kernel look at the same inputs.  Contracts, weights and correlation matrices are
tests/helpers/basket_general_cases.py's (drawn_case, spread_case: imported, not edited); the barriers are
tests/helpers/basket_path_reference.py's default ones (about one sigma sqrt(T) either side of the basket forward, the
worst barrier 1.5 sigma below the lowest forward)."""

from __future__ import annotations

import functools

import numpy as np

from tests.helpers import basket_general_cases as cases
from tests.helpers import basket_path_reference as pr
from tests.helpers import basket_reference as br

SEED, ORD0 = cases.SEED, cases.ORD0
# (A, T, P, B): two sweeps (64 row sums), odd A, A = 8 in column groups, three sweeps (80 row sums) with a partial
# last lane, A = 5 in column groups with a partial chunk
CASES = [(4, 16, 4096, 6), (3, 5, 2048, 6), (8, 2, 2048, 6), (2, 40, 693, 4), (5, 3, 1000, 6)]
# the asset counts those leave out, at the smallest shape that still runs the column groups and the normalisation sweep
# (one stream per group, a ragged lane, a partial chunk): tests/test_instantiation_ledger.py holds the table to the
# ledger of instantiations, and each row below is the only one of its A
LEDGER_CASES = [(1, 3, 693, 3), (6, 3, 693, 3), (7, 3, 693, 3)]
CASES += LEDGER_CASES
SPREAD = (2, 4, 2049, 6)  # weights (1, -1), K = 0: levels of either sign
EPS = {"portable": br.PORTABLE, "hw": br.HW}


@functools.lru_cache(maxsize=None)
def inputs(oracle, A: int, B: int, spread: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(rows [B, 3A + 4], weights [B, A], correlation [B, A, A], barriers [B, 3]).  Read-only: shared by the tests."""
    rows, w, C = cases.spread_case(oracle, B) if spread else cases.drawn_case(oracle, A, B)
    bars = pr.default_barriers(rows, A, w, C)
    for a in (rows, w, C, bars):
        a.setflags(write=False)
    return rows, w, C, bars


@functools.lru_cache(maxsize=None)
def simulated(oracle, A: int, T: int, P: int, B: int, math: str, spread: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """The f64 rows and their bounds of a case in one math mode: computed once, left unchanged."""
    rows, _, C, _ = inputs(oracle, A, B, spread)
    x, rel = pr.simulate(oracle, rows, A, T, P, SEED, ORD0, corr=C, eps=EPS[math])
    x.setflags(write=False)
    rel.setflags(write=False)
    return x, rel


@functools.lru_cache(maxsize=None)
def reference(oracle, A: int, T: int, P: int, B: int, math: str, normalize: bool, spread: bool = False,
              barriers: bool = True) -> pr.PathRef:
    rows, w, _, bars = inputs(oracle, A, B, spread)
    x, rel = simulated(oracle, A, T, P, B, math, spread)
    return pr.outputs(rows, A, x, rel, w, bars if barriers else None, normalize)
