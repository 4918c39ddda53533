"""An independent float64 reference of the Greeks of the weighted, general-correlation basket
(smc_basket_greeks_general), on basket_reference.py's stream words, drivers and paths(..., L=).  numpy only.

What it shares with the kernel: the words of the streams and the documented meaning of the columns
(include/spectralmc_hip.h).  What it does not share: any arithmetic.  The factor is numpy.linalg.cholesky of the
matrix; the Brownian sums come from the drivers, never from the log of a terminal value; the derivative of the factor
in the pair (j, k) is the closed form
    dL / dC_jk = L Phi(L^-1 E_jk L^-T),   E_jk = e_j e_k^T + e_k e_j^T,   Phi = strict lower triangle + half the diagonal,
applied to the driver sums directly (no G = dL L^-1, no folded g_im, no differentiated Banachiewicz recursion, no packed
triangle, no moment sums).

The model
---------
x_i = X0_i exp(mu_i T + v_i W_i), mu_i = r - d_i - v_i^2 / 2, W = L Z, Z_k = sqrt(dt) sum_t z_k(t), C = L L^T.  The
drivers do not depend on C, so dW / dC_jk = (dL / dC_jk) Z, where C_jk and C_kj move together (the matrix stays
symmetric).  Per asset
    d ln x_i / d v_i = W_i - v_i T,   d ln x_i / d T = mu_i + v_i W_i / (2 T),   d ln x_i / d C_jk = v_i (dW / dC_jk)_i,
and d ln x_i / d X0_i = 1 / X0_i, d ln x_i / d r = T.  Under RAW xs_i = x_i.  Under NORMALIZE xs_i = x_i F_i / mean_p(x_i):
for a parameter other than X0 and r the derivative of ln xs_i is that of ln x_i less its x_i-weighted mean over the
paths, plus that of ln F_i (r - d_i for T, 0 otherwise).  The basket is bk = sum_i w_i xs_i with the caller's weights
(any sign), the prices df max(+-(K - bk), 0), so on an exercised path d price / d theta = -+ df sum_i w_i xs_i
d ln xs_i / d theta, plus -T price for r and -r price for T; theta is reported as -d V / d T.

Conventions of the header, applied as stated there: v_i == 0 gives vega_i = 0; any v_i == 0 with A > 1 gives NaN in
every pair column; A == 1 has no pair column; T == 0 keeps mu_i / 2 (RAW) or r - d_i (NORMALIZE) as d ln xs_i / d T.

The block: [B, 2 A^2 + 6 A + 12] in the header's column order (n = 4A + 4 + A (A - 1): deltas, vegas, rho, theta, the
put's pair columns in pack order, the call's, their standard errors, the prices and theirs); the sums
[B, A + A (A + 1) / 2]: sum x_i, then sum_p x_i ln(x_m / X0_m) for m <= i row by row (0 under RAW, as the kernel
reports them).
"""

from __future__ import annotations

import numpy as np

from tests.helpers import basket_general_reference as gen
from tests.helpers import basket_reference as br


def pairs(A: int) -> list[tuple[int, int]]:
    """(j, k), k < j, in pack_correlation's order."""
    return [(j, k) for j in range(A) for k in range(j)]


def cols(A: int) -> int:
    return 2 * A * A + 6 * A + 12


def greek_columns(A: int) -> int:
    return 4 * A + 4 + A * (A - 1)


def matrices(rows: np.ndarray, A: int, corr: np.ndarray | None) -> np.ndarray:
    """C [B, A, A]: the given matrices (one for all, or one each), or the equicorrelation matrix of each row's rho."""
    rows = np.asarray(rows, dtype=np.float64)
    if corr is None:
        rho = br.fields(rows, A)[3]
        return (1.0 - rho)[:, None, None] * np.eye(A) + rho[:, None, None] * np.ones((A, A))
    return np.array(np.broadcast_to(np.asarray(corr, dtype=np.float64), (rows.shape[0], A, A)))


def dfactor_pair(L: np.ndarray, j: int, k: int) -> np.ndarray:
    """d L / d C_jk of the lower Cholesky factor L [A, A], C_jk and C_kj moving together."""
    A = L.shape[0]
    Li = np.linalg.inv(L)
    E = np.zeros((A, A))
    E[j, k] = E[k, j] = 1.0
    S = Li @ E @ Li.T
    return L @ (np.tril(S, -1) + 0.5 * np.diag(np.diag(S)))


def words_and_drivers(oracle, B: int, A: int, T: int, P: int, seed: int, ordinal0: int) -> np.ndarray:
    """z [B, A, T, P] of the contracts' streams."""
    z, _ = br.drivers(br.stream_words(oracle, B, A, T, P, seed, ordinal0))
    return np.ascontiguousarray(z[:, :A, :, :P])


def _terminal(rows: np.ndarray, A: int, T: int, z: np.ndarray, L: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    x, rel = br.paths(rows, A, T, z, np.abs(z), br.PORTABLE, L=L)
    return np.ascontiguousarray(x[:, :, -1, :]), np.ascontiguousarray(rel[:, :, -1, :])


def prices(rows: np.ndarray, A: int, T: int, z: np.ndarray, w: np.ndarray, C: np.ndarray, normalize: bool) -> np.ndarray:
    """[B, 2]: basket_general_reference's own Monte-Carlo put and call on the drivers z [B, A, T, P] (the function the
    Greeks differentiate): its factors, basket_reference's paths, its outputs."""
    L = gen.factors(rows, A, C)
    xT, relT = _terminal(rows, A, T, z, L)
    return gen.outputs(rows, A, xT, relT, w, normalize).cols[:, :2]


def path_terms(rows: np.ndarray, A: int, T: int, z: np.ndarray, w: np.ndarray, C: np.ndarray, normalize: bool, *,
               dfactor=dfactor_pair, drop_ac: bool = False, term_weights: np.ndarray | None = None) -> dict:
    """The per-path terms [n + 2, B, P] in the block's column order (the prices last), the sums, the basket bk [B, P]
    and its derivatives dbk [2A + 2 + np, B, P] with respect to X0_i, v_i, r, T and each C_jk (for the kink bound of a
    finite difference).  dfactor, drop_ac (no NORMALIZE correction of the pair columns) and term_weights (other
    weights on the terms than in the basket) exist for the tests' wrong readings."""
    rows = np.asarray(rows, dtype=np.float64)
    K, Tm, r, _, X0, d, v = br.fields(rows, A)
    B, P = z.shape[0], z.shape[-1]
    pr = pairs(A)
    L = np.stack([np.linalg.cholesky(c) for c in C])
    xT, _ = _terminal(rows, A, T, z, L)
    Z = np.sqrt(Tm / T)[:, None, None] * z.sum(axis=2)                       # [B, A, P]
    W = np.einsum("bik,bkp->bip", L, Z)
    mu = r[:, None] - d - 0.5 * v * v
    col = lambda a: a[:, :, None]  # noqa: E731
    Tcol = col(np.broadcast_to(Tm[:, None], v.shape))
    with np.errstate(divide="ignore", invalid="ignore"):
        dT = np.where(Tcol == 0.0, col(mu / 2.0), col(mu) + col(v) * W / (2.0 * Tm[:, None, None]))
    dv = np.where(col(v) == 0.0, 0.0, W - col(v * Tm[:, None]))
    dC = [col(v) * np.einsum("bik,bkp->bip", np.stack([dfactor(L[b], j, k) for b in range(B)]), Z) for j, k in pr]
    nm = A * (A + 1) // 2
    sums = np.zeros((B, A + nm))
    sums[:, :A] = xT.sum(axis=2)
    xs = xT
    if normalize:
        logs = col(mu * Tm[:, None]) + col(v) * W                             # ln(x_m / X0_m), from the drivers
        sums[:, A:] = np.stack([(xT[:, i] * logs[:, m]).sum(axis=1) for i in range(A) for m in range(i + 1)], axis=1)
        wmean = lambda a: col((xT * a).sum(axis=2) / sums[:, :A])  # noqa: E731
        dv = np.where(col(v) == 0.0, 0.0, dv - wmean(dv))
        dT = dT - wmean(dT) + col(r[:, None] - d)
        dT = np.where(Tcol == 0.0, col(r[:, None] - d), dT)
        if not drop_ac:
            dC = [a - wmean(a) for a in dC]
        xs = xT * col(X0 * np.exp((r[:, None] - d) * Tm[:, None]) / xT.mean(axis=2))
    bk = (col(w) * xs).sum(axis=1)
    df = np.exp(-r * Tm)[:, None]
    ip, ic = K[:, None] - bk > 0.0, bk - K[:, None] > 0.0
    put, call = df * np.where(ip, K[:, None] - bk, 0.0), df * np.where(ic, bk - K[:, None], 0.0)
    tw = w if term_weights is None else term_weights
    wx = df[:, None, :] * xs * col(tw)                                        # [B, A, P]
    both = lambda s: [np.where(ip, -s, 0.0), np.where(ic, s, 0.0)]  # noqa: E731
    t: list[np.ndarray] = []
    t += [np.where(ip, -(wx[:, i] / X0[:, i, None]), 0.0) for i in range(A)]
    t += [np.where(ic, wx[:, i] / X0[:, i, None], 0.0) for i in range(A)]
    t += [np.where(ip, -(wx[:, i] * dv[:, i]), 0.0) for i in range(A)]
    t += [np.where(ic, wx[:, i] * dv[:, i], 0.0) for i in range(A)]
    t += both(np.broadcast_to((Tm * K)[:, None] * df, bk.shape))
    sT = (wx * dT).sum(axis=1)
    t += [r[:, None] * put + np.where(ip, sT, 0.0), r[:, None] * call - np.where(ic, sT, 0.0)]
    dead = np.any(v == 0.0, axis=1)[:, None]
    sC = [(wx * a).sum(axis=1) for a in dC]
    t += [np.where(dead, np.nan, np.where(ip, -s, 0.0)) for s in sC]
    t += [np.where(dead, np.nan, np.where(ic, s, 0.0)) for s in sC]
    t += [put, call]
    wxs = col(w) * xs
    dbk = [wxs[:, i] / X0[:, i, None] for i in range(A)] + [wxs[:, i] * dv[:, i] for i in range(A)]
    dbk += [Tm[:, None] * bk, (wxs * dT).sum(axis=1)] + [(wxs * a).sum(axis=1) for a in dC]
    return {"t": np.stack(t), "sums": sums, "bk": bk, "dbk": np.stack(dbk), "df": df[:, 0], "xT": xT}


def block_of(t: np.ndarray, A: int) -> np.ndarray:
    """[B, 2 A^2 + 6 A + 12] from per-path terms [n + 2, B, P]: means, then standard errors (0 at P = 1), prices last."""
    n = greek_columns(A)
    P = t.shape[2]
    m = t.mean(axis=2)
    se = t.std(axis=2, ddof=1) / np.sqrt(P) if P > 1 else np.where(np.isnan(m), np.nan, 0.0)
    out = np.empty((t.shape[1], cols(A)))
    out[:, :n], out[:, n:2 * n] = m[:n].T, se[:n].T
    out[:, 2 * n:2 * n + 2], out[:, 2 * n + 2:] = m[n:].T, se[n:].T
    return out


def greeks(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, *,
           weights: np.ndarray | None = None, corr: np.ndarray | None = None,
           normalize: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """(block [B, 2 A^2 + 6 A + 12], sums [B, A + A (A + 1) / 2]) of smc_basket_greeks_general for these contracts, in
    float64.  weights [A] or [B, A] (None: 1 / A), corr [A, A] or [B, A, A] (None: each row's rho)."""
    rows = np.asarray(rows, dtype=np.float64)
    B = rows.shape[0]
    w = np.full((B, A), 1.0 / A) if weights is None else np.array(np.broadcast_to(np.asarray(weights, dtype=np.float64), (B, A)))
    C = matrices(rows, A, corr)
    blocks, sums = [], []
    for b0 in range(0, B, br.BLOCK):
        blk = rows[b0:b0 + br.BLOCK]
        z = words_and_drivers(oracle, blk.shape[0], A, T, P, seed, ordinal0 + b0)
        r = path_terms(blk, A, T, z, w[b0:b0 + br.BLOCK], C[b0:b0 + br.BLOCK], normalize)
        blocks.append(block_of(r["t"], A))
        sums.append(r["sums"])
    return np.concatenate(blocks), np.concatenate(sums)


def mean_columns(A: int) -> list[int]:
    """The columns that are means (the Greeks and the two prices)."""
    n = greek_columns(A)
    return list(range(n)) + [2 * n, 2 * n + 1]


def stderr_column(A: int, col: int) -> int:
    """The column holding the standard error of mean column col."""
    n = greek_columns(A)
    return col + n if col < n else col + 2


def unpack(tri: np.ndarray, A: int) -> np.ndarray:
    """Packed rows [.., A (A - 1) / 2] as symmetric [.., A, A] with a zero diagonal."""
    out = np.zeros(tri.shape[:-1] + (A, A))
    for q, (j, k) in enumerate(pairs(A)):
        out[..., j, k] = out[..., k, j] = tri[..., q]
    return out
