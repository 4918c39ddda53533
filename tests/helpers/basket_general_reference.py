"""An independent float64 reference of the weighted, general-correlation basket pricer (basket_general_kernel,
smc_basket_price_general), with an a-priori bound on how far the f32 kernel may lie from it.  numpy only.

It stands on tests/helpers/basket_reference.py (read that docstring first) and imports from it, unchanged: the
drivers (stream words, Box-Muller), paths(..., L=...) with its per-element relative bound, terminal_sums, forwards,
scaled and _payoff.  What is new here is what the new kernel adds to smc_basket_price.

The model
---------
Contract row [3A + 4]: K, T, r, rho, X0[A], d[A], v[A]; beside it a row of A weights w_i (any sign, not normalised;
absent: 1 / A) and a correlation matrix C (symmetric, unit diagonal, positive definite; absent: the equicorrelation
matrix of the row's rho).  The drivers of a step are correlated by C = L L^T with L = numpy.linalg.cholesky(C): not
the kernel's Banachiewicz statements, no packed triangle, no index arithmetic (basket_reference.factor where C is
absent, which also writes out the singular corner A = 2, rho = 1).  Paths, terminal sums tot_i, forwards F_i, the
discount df and the scaled terminal values xs_i are basket_reference's.  Per path
    bk = sum_i w_i xs_i,   mx = max_i xs_i,   mn = min_i xs_i      (mx and mn do not see the weights),
and the 18 columns are smc_basket_price's with this bk: the means of df max(+-(K - u), 0) for u = bk, mx, mn, their
standard errors, the means of bk, mx, mn, the share of paths with bk < K, and the intrinsic values at
Fb = sum_i w_i F_i.

The bound
---------
Nothing is fitted to the kernel.  The inputs are the reference's own intermediate values, U = 2^-24 and the math
epsilons basket_reference already uses (through paths, forwards and scaled).

* Factor: the kernel factors C in f64 (one rounding of 2^-53 per operation, amplified by at most the condition of
  C); against the f32 roundings of the step coefficients, which paths() already carries (relative U on every
  c_k = v sqrt(dt) log2 e L_ik), this is eight orders below and is left out, as basket_reference leaves out its own
  f64 errors.  paths() takes |L_ik| from the L it is given, so its bound holds for any factor.
* Weighted basket.  The kernel forms t_i = f32(w_i) * xs_i and bk = ((0 + t_0) + t_1) + ... in f32, every operation
  rounded.  A term goes through at most A + 1 roundings: one of w_i, one of the product, and the A - 1 additions
  that follow the exact 0 + t_0.  With the kernel's xs_i within delta_xs_i of the reference's, every computed
  quantity that a rounding acts on is at most sum_i |w_i| (|xs_i| + delta_xs_i) in magnitude, so
      delta_bk = sum_i |w_i| delta_xs_i + ((1 + U)^(A + 1) - 1) sum_i |w_i| (|xs_i| + delta_xs_i).
  basket_reference._mean_of has the plain sums where this has absolute values: its partial sums are positive, these
  are not once a weight is negative.  With w_i = 1 / A the two expressions are the same.
* max and min are 1-Lipschitz in the largest delta_xs of the path (unchanged).
* Payoffs, means and standard errors: basket_reference's propagation (its _payoff, and price_columns' formulas for
  the f64 summation and for sum v^2 - P m^2), restated here because price_columns also fixes the equal-weight Fb.
  _payoff charges the rounding of K as U K: the strikes used must be >= 0 (asserted).
* Exercise share: a path can be counted differently only if |K - bk| <= delta_bk + U |K|; the tolerance is the
  number of such reference paths over P, and basket_reference.exercise_count_ok is the condition on the contracts.
* Intrinsic values: Fb = ((0 + w_0 F_0) + w_1 F_1) + ... is the same weighted sum on F_i with F_i's relative bound
  eF_i in place of delta_xs_i.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.helpers import basket_reference as br
from tests.helpers.basket_reference import (U, _payoff, drivers, fields, forwards, paths, scaled, stream_words,
                                            terminal_sums)

BLOCK = br.BLOCK


def factors(rows: np.ndarray, A: int, corr: np.ndarray | None) -> np.ndarray:
    """L [B, A, A] with L L^T = C: numpy.linalg.cholesky of the matrices corr [B, A, A] (or one [A, A] for all), or
    basket_reference.factor of each row's rho where corr is None."""
    rows = np.asarray(rows, dtype=np.float64)
    if corr is None:
        return np.stack([br.factor(A, rho) for rho in fields(rows, A)[3]])
    corr = np.broadcast_to(np.asarray(corr, dtype=np.float64), (rows.shape[0], A, A))
    return np.stack([np.linalg.cholesky(C) for C in corr])


def weighted(xs: np.ndarray, dxs: np.ndarray, w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(sum_i w_i xs_i, its bound) over axis 1 as the kernel forms it; w [B, A] against xs [B, A] or [B, A, P]."""
    A = xs.shape[1]
    w = w.reshape(w.shape + (1,) * (xs.ndim - 2))
    mag = (np.abs(w) * (np.abs(xs) + dxs)).sum(axis=1)
    return (w * xs).sum(axis=1), (np.abs(w) * dxs).sum(axis=1) + ((1.0 + U) ** (A + 1) - 1.0) * mag


def underlyings(xs: np.ndarray, dxs: np.ndarray, w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(u, delta_u) [3, B, P]: the weighted basket, the best and the worst (unweighted) of each path."""
    bk, dbk = weighted(xs, dxs, w)
    worst = dxs.max(axis=1)
    return np.stack([bk, xs.max(axis=1), xs.min(axis=1)]), np.stack([dbk, worst, worst])


def price_columns(rows: np.ndarray, A: int, u: np.ndarray, du: np.ndarray,
                  w: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(columns [B, 18], their bounds [B, 18], exercise counts in doubt [B]) from underlyings(...)."""
    K = fields(rows, A)[0]
    assert np.all(K >= 0.0), "the payoff bound charges U K for the rounding of the strike"
    B, P = u.shape[1], u.shape[2]
    F, eF, df, edf = forwards(rows, A)
    out = [_payoff(sign, K[:, None], u[k], du[k], df[:, None], edf[:, None]) for k in range(3) for sign in (1.0, -1.0)]
    v, dv = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    cols, bound = np.zeros((B, 18)), np.zeros((B, 18))
    cols[:, :6] = v.mean(axis=2).T
    bound[:, :6] = (dv.mean(axis=2) + P * 2.0 ** -52 * v.mean(axis=2)).T
    if P > 1:
        cols[:, 6:12] = (v.std(axis=2, ddof=1) / np.sqrt(P)).T
        H = 4 * P * 2.0 ** -53 * np.square(v + dv).sum(axis=2)
        bound[:, 6:12] = ((np.sqrt(np.square(dv).sum(axis=2)) + np.sqrt(H)) / np.sqrt(P * (P - 1.0))).T
    cols[:, 12:15] = u.mean(axis=2).T
    bound[:, 12:15] = (du.mean(axis=2) + P * 2.0 ** -52 * np.abs(u).mean(axis=2)).T
    cols[:, 15] = (u[0] < K[:, None]).mean(axis=1)
    doubt = (np.abs(K[:, None] - u[0]) <= du[0] + U * np.abs(K)[:, None]).sum(axis=1)
    bound[:, 15] = doubt / P
    Fb, dFb = weighted(F, F * eF, w)
    for col, sign in ((16, 1.0), (17, -1.0)):
        cols[:, col], bound[:, col] = _payoff(sign, K, Fb, dFb, df, edf)
    return cols, bound, doubt


@dataclass
class GeneralRef:
    xT: np.ndarray         # [B, A, P] terminal values
    relT: np.ndarray
    tot: np.ndarray        # [B, A] terminal sums
    tot_bound: np.ndarray
    xs: np.ndarray         # [B, A, P] scaled terminal values
    dxs: np.ndarray
    u: np.ndarray          # [3, B, P] weighted basket, best, worst
    du: np.ndarray
    cols: np.ndarray       # [B, 18]
    cols_bound: np.ndarray
    doubt: np.ndarray      # [B] paths whose exercise the bound leaves open


def outputs(rows: np.ndarray, A: int, xT: np.ndarray, relT: np.ndarray, w: np.ndarray, normalize: bool) -> GeneralRef:
    """Everything downstream of the terminal values (xT, relT) [B, A, P]."""
    tot, tot_bound = terminal_sums(xT, relT)
    F, eF, _, _ = forwards(rows, A)
    xs, dxs = scaled(xT, relT, tot, tot_bound, normalize, F, eF)
    u, du = underlyings(xs, dxs, w)
    cols, cols_bound, doubt = price_columns(rows, A, u, du, w)
    return GeneralRef(xT, relT, tot, tot_bound, xs, dxs, u, du, cols, cols_bound, doubt)


def reference(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, *,
              weights: np.ndarray | None = None, corr: np.ndarray | None = None, L: np.ndarray | None = None,
              normalize: bool = True, eps: br.MathEps = br.PORTABLE) -> GeneralRef:
    """smc_basket_price_general's outputs for these contracts, and their bounds.  weights [A] or [B, A] (None: 1 / A),
    corr [A, A] or [B, A, A] (None: each row's rho); L [B, A, A] overrides the factor (the tests' wrong readings)."""
    rows = np.asarray(rows, dtype=np.float64)
    B = rows.shape[0]
    w = np.full((B, A), 1.0 / A) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), (B, A))
    L = factors(rows, A, corr) if L is None else L
    parts = []
    for b0 in range(0, B, BLOCK):
        blk = rows[b0:b0 + BLOCK]
        z, rad = drivers(stream_words(oracle, blk.shape[0], A, T, P, seed, ordinal0 + b0))
        x, rel = paths(blk, A, T, z[:, :A, :, :P], rad[:, :A, :, :P], eps, L=L[b0:b0 + BLOCK])
        parts.append(outputs(blk, A, np.ascontiguousarray(x[:, :, -1, :]), np.ascontiguousarray(rel[:, :, -1, :]),
                             w[b0:b0 + BLOCK], normalize))
    if len(parts) == 1:
        return parts[0]
    axis = {"u": 1, "du": 1}
    return GeneralRef(**{name: np.concatenate([getattr(p, name) for p in parts], axis=axis.get(name, 0))
                         for name in GeneralRef.__dataclass_fields__})


# ---- the closed form the correlation is checked against --------------------------------------------------------------
def margrabe(rows: np.ndarray) -> np.ndarray:
    """The exchange option df E max(x_0 - x_1, 0) of A = 2 rows (K is not used) under the row's rho:
    df (F_0 Phi(d1) - F_1 Phi(d1 - sigma sqrt(T))), sigma^2 = v_0^2 + v_1^2 - 2 rho v_0 v_1."""
    from math import erf

    _, Tm, r, rho, X0, d, v = fields(rows, 2)
    F = X0 * np.exp((r[:, None] - d) * Tm[:, None])
    sig = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2 - 2.0 * rho * v[:, 0] * v[:, 1]) * np.sqrt(Tm)
    d1 = (np.log(F[:, 0] / F[:, 1]) + 0.5 * sig * sig) / sig
    Phi = lambda a: 0.5 * (1.0 + np.array([erf(t / np.sqrt(2.0)) for t in a]))  # noqa: E731
    return np.exp(-r * Tm) * (F[:, 0] * Phi(d1) - F[:, 1] * Phi(d1 - sig))
