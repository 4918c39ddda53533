"""The table of smc_basket_greeks_general (include/spectralmc_hip.h) in numpy float32, operation by operation: the CPU
expectation of basket_greeks_general_kernel in portable math, for measuring how far float32 takes the columns from the
float64 reference.  Terminal values: a float32 walk of the documented step with the general factor (the portable
Box-Muller of the stream words, the fma chain y_i = a_i + sum_k (b_i L_ik) z_k taken as a float64 product and sum
rounded to float32, x_i *= exp2(y_i)).  Constants in float64 from the contract row in the header's order (the factor,
its derivative per pair and G by the header's recursions in Python floats), then rounded to float32; every per-path
operation is one float32 numpy operation; the sums are float64 in numpy's order, not the kernel's."""

from __future__ import annotations

import numpy as np

from tests.helpers import basket_reference as br

f32 = np.float32
LOG2E = 1.4426950408889634


def factor(A: int, C: np.ndarray) -> list[list[float]]:
    """The engine's Banachiewicz statements on the matrix's lower triangle, in Python floats."""
    L = [[0.0] * A for _ in range(A)]
    for i in range(A):
        for k in range(i + 1):
            s = 1.0 if i == k else float(C[i, k])
            for m in range(k):
                s = s - L[i][m] * L[k][m]
            L[i][k] = (s if s > 0.0 else 0.0) ** 0.5 if i == k else s / L[k][k]
    return L


def g_pair(L: list[list[float]], j: int, k: int) -> np.ndarray:
    """G^jk = (dL / dC_jk) L^-1 by the header's two recursions with the seed at (j, k)."""
    A = len(L)
    dL = [[0.0] * A for _ in range(A)]
    G = [[0.0] * A for _ in range(A)]
    for i in range(A):
        for m in range(i + 1):
            ds = 1.0 if (i == j and m == k) else 0.0
            for u in range(m):
                ds = ds - (dL[i][u] * L[m][u] + L[i][u] * dL[m][u])
            dL[i][m] = ds / (2.0 * L[i][i]) if i == m else (ds - L[i][m] * dL[m][m]) / L[m][m]
    for i in range(A):
        for m in range(i, -1, -1):
            g = dL[i][m]
            for u in range(m + 1, i + 1):
                g = g - G[i][u] * L[u][m]
            G[i][m] = g / L[m][m]
    return np.array(G)


def terminal_values(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, C: np.ndarray) -> np.ndarray:
    """x [B, A, P] float32: the float32 walk of the step with the factor of each contract's matrix C [B, A, A]."""
    rows = np.asarray(rows, dtype=np.float64)
    B = rows.shape[0]
    _, Tm, r, _, X0, d, v = br.fields(rows, A)
    words = br.stream_words(oracle, B, A, T, P, seed, ordinal0)            # [B, G, T, 4, pairs, 2]
    G, pairs = words.shape[1], words.shape[4]
    z = oracle.normal_f32_n(words[..., 0].ravel(), words[..., 1].ravel()).reshape(B, G, T, 4, 2 * pairs)
    z = np.ascontiguousarray(z.transpose(0, 4, 2, 1, 3)).reshape(B, 2 * pairs, T, 4 * G)[:, :A, :, :P]
    dt = Tm / T
    ca = ((r[:, None] - d - 0.5 * v * v) * dt[:, None] * LOG2E).astype(f32)
    x = np.repeat(X0.astype(f32)[:, :, None], P, axis=2)
    for b in range(B):
        L = factor(A, C[b])
        bi = v[b] * np.sqrt(dt[b]) * LOG2E
        for t in range(T):
            for i in range(A):
                y = np.full(P, ca[b, i], dtype=f32)
                for k in range(i + 1):
                    lb = f32(bi[i] * L[i][k])
                    y = (np.float64(lb) * z[b, k, t].astype(np.float64) + y.astype(np.float64)).astype(f32)
                x[b, i] = x[b, i] * oracle.exp2_n(y)
    assert x.dtype == f32
    return x


def restate(oracle, rows: np.ndarray, A: int, x: np.ndarray, w: np.ndarray, C: np.ndarray, norm: bool) -> np.ndarray:
    """The block [B, 2 A^2 + 6 A + 12] from raw terminal values x [B, A, P] float32, weights w [B, A] and matrices C."""
    rows = np.asarray(rows, dtype=np.float64)
    B, _, P = x.shape
    K, Tm, r, _, X0, d, v = br.fields(rows, A)
    pr = [(j, k) for j in range(A) for k in range(j)]
    npr = len(pr)
    Tf, Kf = Tm.astype(f32), K.astype(f32)
    df = oracle.exp_n((-r).astype(f32) * Tf)
    F = X0.astype(f32) * oracle.exp_n(((r[:, None] - d).astype(f32) * Tf[:, None]).ravel()).reshape(B, A)
    mu = r[:, None] - d - 0.5 * v * v
    wt = w.astype(f32)
    dead = np.any(v == 0.0, axis=1)
    g, g0 = np.zeros((B, npr, A, A), dtype=f32), np.zeros((B, npr, A), dtype=f32)
    for b in range(B):
        if dead[b]:
            continue
        L = factor(A, C[b])
        for q, (j, k) in enumerate(pr):
            G = g_pair(L, j, k)
            for i in range(A):
                gs = 0.0
                for m in range(i + 1):
                    gs = gs + G[i, m] * mu[b, m] * Tm[b] / v[b, m]
                    g[b, q, i, m] = f32(v[b, i] * G[i, m] / v[b, m])
                g0[b, q, i] = f32(-(v[b, i] * gs))
    logs = oracle.log_pos_n((x / X0.astype(f32)[:, :, None]).ravel()).reshape(B, A, P)
    tot = x.astype(np.float64).sum(axis=2)
    with np.errstate(all="ignore"):
        ix0 = (1.0 / X0).astype(f32)
        cv = np.where(v == 0, 0.0, 1.0 / v).astype(f32)
        cT = np.where(Tm == 0, 0.0, 1.0 / (2.0 * Tm)).astype(f32)
        ac = np.zeros((B, npr, A), dtype=f32)
        if norm:
            M = np.zeros((B, A, A))
            for i in range(A):
                for m in range(i + 1):
                    M[:, i, m] = (x[:, i] * logs[:, m]).astype(np.float64).sum(axis=1)
            s = F / (tot / float(P)).astype(f32)
            lbar = np.stack([M[:, i, i] for i in range(A)], axis=1) / tot
            av = np.where(v == 0, 0.0, -lbar / v).astype(f32)
            aT = np.where(Tm[:, None] == 0, r[:, None] - d, -lbar / (2.0 * Tm[:, None]) + (r[:, None] - d)).astype(f32)
            for q in range(npr):
                for i in range(A):
                    acc = g0[:, q, i].astype(np.float64)
                    for m in range(i + 1):
                        acc = acc + g[:, q, i, m].astype(np.float64) * (M[:, i, m] / tot[:, i])
                    ac[:, q, i] = (-acc).astype(f32)
        else:
            s = np.ones((B, A), dtype=f32)
            av = np.where(v == 0, 0.0, -mu * Tm[:, None] / v - v * Tm[:, None]).astype(f32)
            aT = (mu / 2.0).astype(f32)
    crho = df * (Tf * Kf)
    rr = r.astype(f32)
    zero = f32(0)
    col = lambda a: a[:, None]  # noqa: E731
    xs = x * s[:, :, None]
    bk = np.zeros((B, P), dtype=f32)
    for i in range(A):
        bk = bk + col(wt[:, i]) * xs[:, i]
    dp, dc = col(Kf) - bk, bk - col(Kf)
    ip, ic = dp > zero, dc > zero
    put, call = col(df) * np.where(ip, dp, zero), col(df) * np.where(ic, dc, zero)
    wx = [(col(df) * xs[:, i]) * col(wt[:, i]) for i in range(A)]
    sT = np.zeros((B, P), dtype=f32)
    dput, dcall, vput, vcall = [], [], [], []
    for i in range(A):
        wd = wx[i] * col(ix0[:, i])
        wv = wx[i] * (logs[:, i] * col(cv[:, i]) + col(av[:, i]))
        sT = sT + wx[i] * (logs[:, i] * col(cT) + col(aT[:, i]))
        dput.append(np.where(ip, -wd, zero))
        dcall.append(np.where(ic, wd, zero))
        vput.append(np.where(ip, -wv, zero))
        vcall.append(np.where(ic, wv, zero))
    pput, pcall = [], []
    for q, (j, _) in enumerate(pr):
        sC = np.zeros((B, P), dtype=f32)
        for i in range(j, A):
            ci = np.broadcast_to(col(g0[:, q, i]), (B, P)).astype(f32)
            for m in range(i + 1):
                ci = ci + col(g[:, q, i, m]) * logs[:, m]
            sC = sC + wx[i] * (ci + col(ac[:, q, i]))
        pput.append(np.where(ip, -sC, zero))
        pcall.append(np.where(ic, sC, zero))
    cr = np.broadcast_to(col(crho), (B, P))
    t = np.stack(dput + dcall + vput + vcall + [np.where(ip, -cr, zero), np.where(ic, cr, zero),
                                                col(rr) * put + np.where(ip, sT, zero),
                                                col(rr) * call - np.where(ic, sT, zero)] + pput + pcall + [put, call])
    assert t.dtype == f32
    n = 4 * A + 4 + 2 * npr
    t64 = t.astype(np.float64)
    m = t64.sum(axis=2) / P
    D = np.maximum((t64 * t64).sum(axis=2) - P * m * m, 0.0)
    se = np.sqrt(D / (P - 1) / P) if P > 1 else np.zeros_like(m)
    out = np.empty((B, 2 * n + 4))
    out[:, :n], out[:, n:2 * n] = m[:n].T, se[:n].T
    out[:, 2 * n:2 * n + 2], out[:, 2 * n + 2:] = m[n:].T, se[n:].T
    if A > 1:
        out[dead, 4 * A + 4:n] = np.nan
        out[dead, n + 4 * A + 4:2 * n] = np.nan
    return out
