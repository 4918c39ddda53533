"""An independent float64 reference of the basket Greeks (smc_basket_greeks), on basket_reference.py's stream words,
drivers and paths.  numpy only.

What it shares with the kernel: the words of the streams and the documented meaning of the columns
(include/spectralmc_hip.h).  What it does not share: any arithmetic.  The Brownian sums come from the drivers, not
from the logs of the terminal values; the derivative of the Cholesky factor is the closed form
    dLc / drho = Lc Phi(Lc^-1 (11^T - I) Lc^-T),   Phi = strict lower triangle + half the diagonal,
applied to the driver sums directly (no G = dLc Lc^-1, no folded g_ik, no differentiated Banachiewicz recursion, no
log2 units).

The model
---------
x_i = X0_i exp(mu_i T + v_i W_i), mu_i = r - d_i - v_i^2 / 2, W = Lc Z, Z_k = sqrt(dt) sum_t z_k(t).  With the factor's
derivative, dW / drho = (dLc / drho) Z.  Per asset
    d ln x_i / d v_i = W_i - v_i T,   d ln x_i / d T = mu_i + v_i W_i / (2 T),   d ln x_i / d rho = v_i (dW / drho)_i,
and d ln x_i / d X0_i = 1 / X0_i, d ln x_i / d r = T.  Under RAW xs_i = x_i.  Under NORMALIZE xs_i = x_i F_i / mean_p(x_i)
with F_i = X0_i e^{(r - d_i) T}: for a parameter other than X0 and r the derivative of ln xs_i is that of ln x_i less its
x_i-weighted mean over the paths, plus that of ln F_i (r - d_i for T, 0 for v_i and rho); for X0_i it stays 1 / X0_i and
for r it stays T.  The basket is bk = (1 / A) sum_i xs_i, the prices df max(+-(K - bk), 0) with df = e^{-r T}, so on an
exercised path d price / d theta = -+ df (1 / A) sum_i xs_i d ln xs_i / d theta, plus -T price for r and -r price for T.
Hence d V / d r = -+ T K df on the exercised paths in both modes; theta is reported as -d V / d T.

Conventions of the header, applied here as stated there: v_i == 0 gives vega_i = 0 (error 0); any v_i == 0 with A > 1
gives NaN in the four correlation columns; A == 1 gives correlation 0; T == 0 keeps mu_i / 2 (RAW) or r - d_i
(NORMALIZE) as d ln xs_i / d T.

The block: [B, 8A + 16] in the header's column order; the sums [B, 3, A]: sum x_i, sum x_i ln(x_i / X0_i),
sum x_i v_i (dW / drho)_i (the last two 0 under RAW, as the kernel reports them).
"""

from __future__ import annotations

import numpy as np

from tests.helpers import basket_reference as br


def cols(A: int) -> int:
    return 8 * A + 16


def dfactor(A: int, rho: float) -> np.ndarray:
    """d Lc / d rho of the lower Cholesky factor of the equicorrelation matrix (NaN where it is singular)."""
    if A == 1:
        return np.zeros((1, 1))
    Lc = br.factor(A, rho)
    try:
        Li = np.linalg.inv(Lc)
    except np.linalg.LinAlgError:
        return np.full((A, A), np.nan)
    S = Li @ (np.ones((A, A)) - np.eye(A)) @ Li.T
    return Lc @ (np.tril(S, -1) + 0.5 * np.diag(np.diag(S)))


def words_and_drivers(oracle, B: int, A: int, T: int, P: int, seed: int, ordinal0: int) -> tuple[np.ndarray, np.ndarray]:
    """(z, radius) [B, A, T, P] of the contracts' streams."""
    z, rad = br.drivers(br.stream_words(oracle, B, A, T, P, seed, ordinal0))
    return np.ascontiguousarray(z[:, :A, :, :P]), np.ascontiguousarray(rad[:, :A, :, :P])


def _terminal(rows: np.ndarray, A: int, T: int, z: np.ndarray) -> np.ndarray:
    x, _ = br.paths(rows, A, T, z, np.abs(z), br.PORTABLE)  # the bound is not used here
    return np.ascontiguousarray(x[:, :, -1, :])


def prices(rows: np.ndarray, A: int, T: int, z: np.ndarray, normalize: bool) -> np.ndarray:
    """[B, 2]: the Monte-Carlo basket put and call of the drivers z [B, A, T, P] (the function the Greeks differentiate)."""
    K, Tm, r, _, X0, d, _ = br.fields(rows, A)
    xT = _terminal(rows, A, T, z)
    if normalize:
        xT = xT * (X0 * np.exp((r[:, None] - d) * Tm[:, None]) / xT.mean(axis=2))[:, :, None]
    bk = xT.mean(axis=1)
    df = np.exp(-r * Tm)[:, None]
    return np.stack([(df * np.maximum(K[:, None] - bk, 0.0)).mean(axis=1),
                     (df * np.maximum(bk - K[:, None], 0.0)).mean(axis=1)], axis=1)


def path_terms(rows: np.ndarray, A: int, T: int, z: np.ndarray, normalize: bool) -> dict[str, np.ndarray]:
    """The per-path terms [4A + 8, B, P] in the block's column order (the prices last), the sums [B, 3, A], the basket
    bk [B, P] and its derivatives dbk [2A + 3, B, P] with respect to X0_i, v_i, r, T, rho (for the kink bound of a
    finite difference)."""
    rows = np.asarray(rows, dtype=np.float64)
    K, Tm, r, rho, X0, d, v = br.fields(rows, A)
    B, P = z.shape[0], z.shape[-1]
    xT = _terminal(rows, A, T, z)
    Z = np.sqrt(Tm / T)[:, None, None] * z.sum(axis=2)                       # [B, A, P]
    W = np.einsum("bik,bkp->bip", np.stack([br.factor(A, rh) for rh in rho]), Z)
    dW = np.einsum("bik,bkp->bip", np.stack([dfactor(A, rh) for rh in rho]), Z)
    mu = r[:, None] - d - 0.5 * v * v
    col = lambda a: a[:, :, None]  # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        half = np.where(col(np.broadcast_to(Tm[:, None], v.shape)) == 0.0, col(mu / 2.0),
                        col(mu) + col(v) * W / (2.0 * Tm[:, None, None]))
    dv = np.where(col(v) == 0.0, 0.0, W - col(v * Tm[:, None]))
    dT = half
    dr = col(v) * dW
    sums = np.zeros((B, 3, A))
    sums[:, 0] = xT.sum(axis=2)
    xs = xT
    if normalize:
        sums[:, 1] = (xT * np.log(xT / col(X0))).sum(axis=2)
        sums[:, 2] = (xT * dr).sum(axis=2)
        wmean = lambda a: col((xT * a).sum(axis=2) / sums[:, 0])  # noqa: E731
        dv = np.where(col(v) == 0.0, 0.0, dv - wmean(dv))
        dT = dT - wmean(dT) + col(r[:, None] - d)
        if np.any(Tm == 0.0):
            dT = np.where(col(np.broadcast_to(Tm[:, None], v.shape)) == 0.0, col(r[:, None] - d), dT)
        dr = dr - wmean(dr)
        xs = xT * col(X0 * np.exp((r[:, None] - d) * Tm[:, None]) / xT.mean(axis=2))
    bk = xs.mean(axis=1)
    df = np.exp(-r * Tm)[:, None]
    ip, ic = K[:, None] - bk > 0.0, bk - K[:, None] > 0.0
    put, call = df * np.where(ip, K[:, None] - bk, 0.0), df * np.where(ic, bk - K[:, None], 0.0)
    w = df[:, None, :] * xs / A                                               # [B, A, P]
    both = lambda s: [np.where(ip, -s, 0.0), np.where(ic, s, 0.0)]  # noqa: E731
    t: list[np.ndarray] = []
    t += [np.where(ip, -(w[:, i] / X0[:, i, None]), 0.0) for i in range(A)]
    t += [np.where(ic, w[:, i] / X0[:, i, None], 0.0) for i in range(A)]
    t += [np.where(ip, -(w[:, i] * dv[:, i]), 0.0) for i in range(A)]
    t += [np.where(ic, w[:, i] * dv[:, i], 0.0) for i in range(A)]
    t += both(np.broadcast_to((Tm * K)[:, None] * df, bk.shape))
    sT = (w * dT).sum(axis=1)
    t += [r[:, None] * put + np.where(ip, sT, 0.0), r[:, None] * call - np.where(ic, sT, 0.0)]
    sC = (w * dr).sum(axis=1)
    corr = both(sC)
    dead = np.any(v == 0.0, axis=1)
    for k in range(2):
        corr[k] = np.zeros_like(bk) if A == 1 else np.where(dead[:, None], np.nan, corr[k])
    t += corr + [put, call]
    # d bk / d theta (d r: T bk in both modes)
    dbk = [xs[:, i] / A / X0[:, i, None] for i in range(A)] + [xs[:, i] * dv[:, i] / A for i in range(A)]
    dbk += [Tm[:, None] * bk, (xs * dT).sum(axis=1) / A, (xs * dr).sum(axis=1) / A]
    return {"t": np.stack(t), "sums": sums, "bk": bk, "dbk": np.stack(dbk), "df": df[:, 0]}


def block_of(t: np.ndarray, A: int) -> np.ndarray:
    """[B, 8A + 16] from per-path terms [4A + 8, B, P]: means, then standard errors (0 at P = 1), prices last."""
    n = 4 * A + 6
    P = t.shape[2]
    m = t.mean(axis=2)
    se = t.std(axis=2, ddof=1) / np.sqrt(P) if P > 1 else np.where(np.isnan(m), np.nan, 0.0)
    out = np.empty((t.shape[1], cols(A)))
    out[:, :n], out[:, n:2 * n] = m[:n].T, se[:n].T
    out[:, 2 * n:2 * n + 2], out[:, 2 * n + 2:] = m[n:].T, se[n:].T
    return out


def greeks(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, *,
           normalize: bool = True) -> tuple[np.ndarray, np.ndarray]:
    """(block [B, 8A + 16], sums [B, 3, A]) of smc_basket_greeks for these contracts, in float64."""
    rows = np.asarray(rows, dtype=np.float64)
    blocks, sums = [], []
    for b0 in range(0, rows.shape[0], br.BLOCK):
        blk = rows[b0:b0 + br.BLOCK]
        z, _ = words_and_drivers(oracle, blk.shape[0], A, T, P, seed, ordinal0 + b0)
        r = path_terms(blk, A, T, z, normalize)
        blocks.append(block_of(r["t"], A))
        sums.append(r["sums"])
    return np.concatenate(blocks), np.concatenate(sums)


def mean_columns(A: int) -> list[int]:
    """The columns that are means (the Greeks and the two prices)."""
    n = 4 * A + 6
    return list(range(n)) + [2 * n, 2 * n + 1]


def stderr_column(A: int, col: int) -> int:
    """The column holding the standard error of mean column col."""
    n = 4 * A + 6
    return col + n if col < n else col + 2
