"""The contracts, weights and correlation matrices the tests of smc_basket_price_general share (numpy only), so
that the CPU tests of the reference and the GPU tests of the kernel look at the same inputs.

Rows are Sobol-drawn over the default basket bounds as in tests/test_gpu_basket_reference.py; weights are
Dirichlet(1), one row per contract; a correlation matrix is G G^T + diag(U(0.3, 1)) rescaled to a unit diagonal, G an
A x max(2, A / 2) standard normal matrix (smallest eigenvalues 0.07 to 0.36 for the seeds used); K is reset to
sum_i w_i F_i times a factor in [0.8, 1.25], so every payoff is live."""

from __future__ import annotations

import numpy as np

from spectralmc_amd.basket import BasketConfig
from tests.helpers import basket_reference as br

SEED = 7
ORD0 = 3
# (A, T, P, normalize, B): lds with two chunks, odd A, A = 8, a partial chunk, RAW, replay by itself
CASES = [(4, 16, 4096, 1, 6), (3, 5, 2048, 1, 6), (8, 2, 2048, 1, 6), (2, 4, 693, 1, 6), (5, 3, 1000, 0, 6),
         (2, 3, 65536, 1, 3)]
# every other (A, normalisation), at the smallest shape that still runs the park block and the normalisation sweep
# (one stream per group, a ragged lane, a partial chunk): tests/test_instantiation_ledger.py holds the table to the
# ledger of instantiations, and each row below is the only one of its (A, normalisation)
LEDGER_CASES = [(A, 3, 693, 1, 3) for A in (1, 5, 6, 7)] + [(A, 3, 693, 0, 3) for A in (1, 2, 3, 4, 6, 7, 8)]
CASES += LEDGER_CASES


def sobol_rows(oracle, A: int, n: int, skip: int = 0) -> np.ndarray:
    oracle.build()
    lo, hi = BasketConfig(n_assets=A, network_size=64, batches_per_mc_run=32).arrays()
    return oracle.sobol_contracts(SEED, skip, n, lo, hi)


def correlations(rng: np.random.Generator, B: int, A: int) -> np.ndarray:
    """[B, A, A] symmetric, unit diagonal, positive definite."""
    out = np.empty((B, A, A))
    for b in range(B):
        G = rng.standard_normal((A, max(2, A // 2)))
        C = G @ G.T + np.diag(rng.uniform(0.3, 1.0, A))
        s = 1.0 / np.sqrt(np.diag(C))
        C = C * s[:, None] * s[None, :]
        C = 0.5 * (C + C.T)
        np.fill_diagonal(C, 1.0)
        out[b] = C
    return out


def pack(C: np.ndarray) -> np.ndarray:
    """The strict lower triangle of [..., A, A] row by row: (1,0), (2,0), (2,1), (3,0), ..."""
    A = C.shape[-1]
    return np.ascontiguousarray(np.stack([C[..., i, k] for i in range(A) for k in range(i)], axis=-1)
                                if A > 1 else np.zeros(C.shape[:-2] + (0,)))


def strikes_at_the_forward(rows: np.ndarray, A: int, w: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """rows with K reset to sum_i w_i F_i times a factor in [0.8, 1.25]."""
    rows = rows.copy()
    F = br.forwards(rows, A)[0]
    rows[:, 0] = (w * F).sum(axis=1) * rng.uniform(0.8, 1.25, rows.shape[0])
    return rows


def drawn_case(oracle, A: int, B: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(rows [B, 3A + 4], weights [B, A], correlation [B, A, A]) of the case with A assets."""
    rng = np.random.default_rng(2028 + A)
    w = rng.dirichlet(np.ones(A), B)
    C = correlations(rng, B, A)
    return strikes_at_the_forward(sobol_rows(oracle, A, B), A, w, rng), w, C


def spread_case(oracle, B: int = 6) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A = 2, weights (1, -1), K = 0: the exchange option on Sobol-drawn rows under a drawn correlation."""
    rng = np.random.default_rng(2030)
    rows = sobol_rows(oracle, 2, B)
    rows[:, 0] = 0.0
    return rows, np.tile([1.0, -1.0], (B, 1)), correlations(rng, B, 2)


def margrabe_rows() -> np.ndarray:
    """The 32 exchange-option contracts (A = 2, weights (1, -1), K = 0, the rows' own rho) of the Margrabe tests."""
    rng = np.random.default_rng(2028)
    n = 32
    x1 = rng.uniform(80.0, 120.0, n)
    x0 = x1 * rng.uniform(0.9, 1.1, n)
    Tm = rng.uniform(0.25, 2.0, n)
    r = rng.uniform(-0.02, 0.08, n)
    d = rng.uniform(0.0, 0.04, (n, 2))
    v = rng.uniform(0.1, 0.6, (n, 2))
    rho = rng.uniform(-0.9, 0.9, n)
    return np.column_stack([np.zeros(n), Tm, r, rho, x0, x1, d, v])


MARGRABE = dict(T=4, P=16384, seed=7, ordinal0=3)
