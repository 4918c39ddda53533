"""The shapes, contracts, weights and correlation matrices the tests of smc_basket_greeks_paths share (numpy only), so
that the CPU tests of the reference and the GPU tests of the kernel look at the same inputs.

Contract rows are near the money with every v_i sqrt(T) >= 0.1 (tests/helpers/path_greeks_cases.py's rule: the
pathwise estimator's indicator and the row of an extreme are then open on few paths): X0_i in [60, 140], d_i in
[0, 0.04], v_i in [0.15, 0.5], T in [0.5, 2], r in [-0.01, 0.06], K = sum_i w_i F_i times a factor in [0.9, 1.1].
Weights are Dirichlet(1) rows, correlation matrices tests/helpers/basket_general_cases.py's (one per contract).  The
spread case has weights (1, -0.5) and K at the spread's forward plus a tenth of the long leg."""

from __future__ import annotations

import functools

import numpy as np

from tests.helpers import basket_general_cases as cases
from tests.helpers import basket_path_greeks_reference as pg
from tests.helpers import basket_reference as br

SEED, ORD0 = cases.SEED, cases.ORD0
# (A, T, P, B).  Pass plans: A <= 4 takes two payoff simulations, A = 5..8 four (both sides of that layout: A = 4 and
# A = 5).  NORMALIZE sweeps hold floor((144 KiB - 3328 - tables) / (8192 A)) dates: 4 at A = 4 (T = 16: four full
# sweeps; T = 6: a short last sweep of 2), 5 at A = 3 (T = 5: one sweep), 2 at A = 8 (T = 3: a short last sweep of 1),
# 8 at A = 2 (T = 40: five full sweeps), 3 at A = 5 (T = 3: one sweep; T = 4: a short last sweep of 1), 17 at A = 1,
# 2 at A = 6 and A = 7 (T = 3: short last sweeps).  P = 693 and P = 1000 end in a partial lane and a partial chunk.
CASES = [(4, 16, 4096, 6), (3, 5, 2048, 6), (8, 3, 2048, 6), (2, 40, 693, 4), (5, 3, 1000, 6), (4, 6, 693, 4),
         (5, 4, 2048, 4), (1, 7, 2049, 4), (6, 3, 1000, 3), (7, 3, 693, 3)]
SPREAD = (2, 4, 2049, 6)
MATHS = ("portable", "hw")


@functools.lru_cache(maxsize=None)
def inputs(A: int, B: int, spread: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(rows [B, 3A + 4], weights [B, A], correlation [B, A, A]).  Read-only: shared by the tests."""
    rng = np.random.default_rng(4100 + A + (50 if spread else 0))
    w = np.tile([1.0, -0.5], (B, 1)) if spread else rng.dirichlet(np.ones(A), B)
    C = cases.correlations(rng, B, A)
    X0, d = rng.uniform(60.0, 140.0, (B, A)), rng.uniform(0.0, 0.04, (B, A))
    v, Tm, r = rng.uniform(0.15, 0.5, (B, A)), rng.uniform(0.5, 2.0, B), rng.uniform(-0.01, 0.06, B)
    rows = np.column_stack([np.zeros(B), Tm, r, np.zeros(B), X0, d, v])
    F = br.forwards(rows, A)[0]
    if spread:
        rows[:, 0] = (w * F).sum(axis=1) + 0.1 * F[:, 0] * rng.uniform(-1.0, 1.0, B)
    else:
        rows[:, 0] = (w * F).sum(axis=1) * rng.uniform(0.9, 1.1, B)
    assert np.all(v * np.sqrt(Tm)[:, None] >= 0.1)
    for a in (rows, w, C):
        a.setflags(write=False)
    return rows, w, C


def flat_inputs(A: int = 3) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One flat contract (every v_i = 0, r = d_i, X0_i f32 numbers): every row stays on X0 exactly."""
    X0 = np.array([96.0, 128.0, 80.0, 112.0, 64.0, 100.0, 72.0, 144.0])[:A]
    rows = np.concatenate([[100.0, 2.0, 0.03, 0.0], X0, np.full(A, 0.03), np.zeros(A)])[None, :]
    return rows, np.full((1, A), 1.0 / A), np.eye(A)[None]


@functools.lru_cache(maxsize=None)
def draws(oracle, A: int, T: int, P: int, B: int, spread: bool = False) -> tuple[np.ndarray, np.ndarray]:
    rows = inputs(A, B, spread)[0]
    z, rad = pg.draws(oracle, rows, A, T, P, SEED, ORD0)
    z.setflags(write=False)
    rad.setflags(write=False)
    return z, rad


@functools.lru_cache(maxsize=None)
def reference(oracle, A: int, T: int, P: int, B: int, math: str, normalize: bool,
              spread: bool = False) -> pg.BasketPathGreeksRef:
    """The reference of a case in one math mode and normalisation: computed once, left unchanged."""
    rows, w, C = inputs(A, B, spread)
    z, rad = draws(oracle, A, T, P, B, spread)
    return pg.greeks(rows, A, T, z, rad, w, np.linalg.cholesky(C), math, normalize=normalize)
