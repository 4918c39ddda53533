"""The table of smc_basket_greeks (include/spectralmc_hip.h) in numpy float32, operation by operation, on given raw
terminal values: the CPU expectation of basket_greeks_kernel in portable math.  Constants are taken in float64 from the
contract row in the header's order of operations (Python floats are IEEE doubles; the Banachiewicz factor is the
oracle's restatement of the engine's), then rounded to float32; every per-path operation is one float32 numpy
operation; the sums are float64 in numpy's pairwise order, not the kernel's: hence the P 2^-52 bounds of summary()."""

from __future__ import annotations

import numpy as np

f32 = np.float32


def g_matrix(Lc: np.ndarray) -> np.ndarray:
    """G = (dLc / drho) Lc^-1 by the header's two recursions, in float64 scalars."""
    A = Lc.shape[0]
    L = [[float(Lc[i, k]) for k in range(A)] for i in range(A)]
    dL = [[0.0] * A for _ in range(A)]
    G = [[0.0] * A for _ in range(A)]
    with np.errstate(all="ignore"):
        for i in range(A):
            for k in range(i + 1):
                ds = np.float64(0.0 if i == k else 1.0)
                for m in range(k):
                    ds = ds - (dL[i][m] * L[k][m] + L[i][m] * dL[k][m])
                dL[i][k] = ds / np.float64(2.0 * L[i][i]) if i == k else (ds - L[i][k] * dL[k][k]) / np.float64(L[k][k])
        for i in range(A):
            for k in range(i, -1, -1):
                g = np.float64(dL[i][k])
                for m in range(k + 1, i + 1):
                    g = g - G[i][m] * L[m][k]
                G[i][k] = g / np.float64(L[k][k])
    return np.array(G, dtype=np.float64)


def constants(oracle, rows: np.ndarray, A: int, norm: int, sums: np.ndarray, P: int) -> dict[str, np.ndarray]:
    """The header's per-contract constants, float32 [B] or [B, A] (g: [B, A, A]); sums [B, 3, A] are tot, sxl, sxc."""
    rows = np.asarray(rows, dtype=np.float64)
    B = rows.shape[0]
    K, Tm, r, rho = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    X0, d, v = rows[:, 4:4 + A], rows[:, 4 + A:4 + 2 * A], rows[:, 4 + 2 * A:]
    Tf, Kf = Tm.astype(f32), K.astype(f32)
    df = oracle.exp_n((-r).astype(f32) * Tf)
    F = X0.astype(f32) * oracle.exp_n(((r[:, None] - d).astype(f32) * Tf[:, None]).ravel()).reshape(B, A)
    mu = r[:, None] - d - 0.5 * v * v
    g, g0 = np.zeros((B, A, A), dtype=f32), np.zeros((B, A), dtype=f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            if np.any(v[b] == 0.0):
                continue
            G = g_matrix(oracle.basket_cholesky(A, float(rho[b])))
            for i in range(A):
                gs = np.float64(0.0)
                for k in range(i + 1):
                    g[b, i, k] = f32(v[b, i] * G[i, k] / v[b, k])
                    gs = gs + G[i, k] * mu[b, k] * Tm[b] / v[b, k]
                g0[b, i] = f32(-(v[b, i] * gs))
        ix0 = (1.0 / X0).astype(f32)
        cv = np.where(v == 0, 0.0, 1.0 / v).astype(f32)
        cT = np.where(Tm == 0, 0.0, 1.0 / (2.0 * Tm)).astype(f32)
        if norm:
            tot, sxl, sxc = sums[:, 0], sums[:, 1], sums[:, 2]
            s = F / (tot / float(P)).astype(f32)
            lbar = sxl / tot
            av = np.where(v == 0, 0.0, -lbar / v).astype(f32)
            aT = np.where(Tm[:, None] == 0, r[:, None] - d, -lbar / (2.0 * Tm[:, None]) + (r[:, None] - d)).astype(f32)
            ac = (-sxc / tot).astype(f32)
        else:
            s = np.ones((B, A), dtype=f32)
            av = np.where(v == 0, 0.0, -mu * Tm[:, None] / v - v * Tm[:, None]).astype(f32)
            aT = (mu / 2.0).astype(f32)
            ac = np.zeros((B, A), dtype=f32)
    out = {"K": Kf, "df": df, "F": F, "s": s, "wA": f32(1.0 / A), "ix0": ix0, "cv": cv, "cT": cT, "crho": df * (Tf * Kf),
           "rr": r.astype(f32), "g": g, "g0": g0, "av": av, "aT": aT, "ac": ac, "x0": X0.astype(f32),
           "dead": np.any(v == 0.0, axis=1)}
    assert all(a.dtype == f32 for k, a in out.items() if k not in ("dead", "wA"))
    return out


def logs_and_c(oracle, x: np.ndarray, k: dict[str, np.ndarray]) -> tuple[np.ndarray, np.ndarray]:
    """(L, c) [B, A, P] float32: L_i = log_pos(x_i / f32(X0_i)), c_i = g0_i + sum_{k <= i} g_ik L_k in k order."""
    B, A, P = x.shape
    assert x.dtype == f32
    q = x / k["x0"][:, :, None]
    L = oracle.log_pos_n(q.ravel()).reshape(B, A, P)
    c = np.empty_like(L)
    for i in range(A):
        ci = np.broadcast_to(k["g0"][:, i, None], (B, P)).astype(f32)
        for kk in range(i + 1):
            ci = ci + k["g"][:, i, kk, None] * L[:, kk]
        c[:, i] = ci
    assert L.dtype == f32 and c.dtype == f32
    return L, c


def pass1_terms(x: np.ndarray, L: np.ndarray, c: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The per-path terms of sxl and sxc, float64 [B, A, P]: f64(x L) and f64(x c) of float32 products."""
    return (x * L).astype(np.float64), (x * c).astype(np.float64)


def terms(x: np.ndarray, L: np.ndarray, c: np.ndarray, k: dict[str, np.ndarray], A: int) -> np.ndarray:
    """The 4A + 8 per-path terms [4A + 8, B, P] float32 in the block's column order, the prices last."""
    B, _, P = x.shape
    zero = f32(0)
    col = lambda a: a[:, None]  # noqa: E731
    xs = x * k["s"][:, :, None]
    bs = np.zeros((B, P), dtype=f32)
    for i in range(A):
        bs = bs + xs[:, i]
    bk = bs * k["wA"]
    dp, dc = col(k["K"]) - bk, bk - col(k["K"])
    ip, ic = dp > zero, dc > zero
    put = col(k["df"]) * np.where(ip, dp, zero)
    call = col(k["df"]) * np.where(ic, dc, zero)
    sT, sC = np.zeros((B, P), dtype=f32), np.zeros((B, P), dtype=f32)
    dput, dcall, vput, vcall = [], [], [], []
    for i in range(A):
        w = (col(k["df"]) * xs[:, i]) * k["wA"]
        wd = w * col(k["ix0"][:, i])
        wv = w * (L[:, i] * col(k["cv"][:, i]) + col(k["av"][:, i]))
        sT = sT + w * (L[:, i] * col(k["cT"]) + col(k["aT"][:, i]))
        sC = sC + w * (c[:, i] + col(k["ac"][:, i]))
        dput.append(np.where(ip, -wd, zero))
        dcall.append(np.where(ic, wd, zero))
        vput.append(np.where(ip, -wv, zero))
        vcall.append(np.where(ic, wv, zero))
    crho = np.broadcast_to(col(k["crho"]), (B, P))
    t = np.stack(dput + dcall + vput + vcall + [
        np.where(ip, -crho, zero), np.where(ic, crho, zero),
        col(k["rr"]) * put + np.where(ip, sT, zero), col(k["rr"]) * call - np.where(ic, sT, zero),
        np.where(ip, -sC, zero), np.where(ic, sC, zero), put, call])
    assert t.dtype == f32 and t.shape[0] == 4 * A + 8
    return t


def summary(t: np.ndarray, A: int, dead: np.ndarray) -> dict[str, np.ndarray]:
    """From the terms [4A + 8, B, P]: the block [B, 8A + 16] (float64 sums; NaN in the correlation columns of
    contracts with a deterministic asset when A > 1), and per term [4A + 8, B] the sum-order bound of its mean,
    P 2^-52 sum|term| / P, and the quantities of check_stderr."""
    n, P = 4 * A + 6, t.shape[2]
    t64 = t.astype(np.float64)
    s1, s2, sa = t64.sum(axis=2), (t64 * t64).sum(axis=2), np.abs(t64).sum(axis=2)
    m = s1 / P
    D = np.maximum(s2 - P * m * m, 0.0)
    se = np.sqrt(D / (P - 1) / P) if P > 1 else np.zeros_like(m)
    cols = np.empty((t.shape[1], 8 * A + 16))
    cols[:, :n], cols[:, n:2 * n] = m[:n].T, se[:n].T
    cols[:, 2 * n:2 * n + 2], cols[:, 2 * n + 2:] = m[n:].T, se[n:].T
    if A > 1:
        for col in (4 * A + 4, 4 * A + 5, n + 4 * A + 4, n + 4 * A + 5):
            cols[dead, col] = np.nan
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.square(sa / P) / (D / P)
    return {"cols": cols, "bound": P * 2.0 ** -52 * sa / P, "dD": P * 2.0 ** -52 * (s2 + 2 * sa * sa / P), "D": D,
            "rho": rho}


def check_stderr(got: np.ndarray, want: np.ndarray, summ: dict[str, np.ndarray], term: int, P: int, what: str) -> float:
    """tests/test_gpu_greeks.py's _check_stderr: D = sum v^2 - P m^2 moves by e (1 + 3 rho) D with e = P 2^-52 and
    rho = (mean |v|)^2 / var, halved by the square root: within 8 e max(1, rho / 2) relative; where D is not above
    four times its absolute movement dD (every path gives the same term), within sqrt(dD / ((P - 1) P)).  Returns the
    largest share of the bound used."""
    e = P * 2.0 ** -52
    D, dD, rho = summ["D"][term], summ["dD"][term], summ["rho"][term]
    flat = D <= 4 * dD
    with np.errstate(invalid="ignore"):
        tol = np.where(flat, np.sqrt(dD / max(P - 1, 1) / P), 8 * e * np.maximum(1.0, rho / 2) * np.abs(want))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / tol)
    assert np.all(err <= tol), (what, int(np.argmax(share)), float(np.max(share)))
    return float(share.max())


def term_columns(A: int, term: int) -> tuple[int, int]:
    """(mean column, standard-error column) of per-path term `term` (0 .. 4A + 7)."""
    n = 4 * A + 6
    return (term, n + term) if term < n else (n + term, n + term + 2)


def restate(oracle, rows: np.ndarray, A: int, x: np.ndarray, norm: int, sums: np.ndarray | None = None) -> dict:
    """The whole block from raw terminal values x [B, A, P] float32.  sums [B, 3, A]: the pass-1 sums the constants are
    taken from (the kernel's own, in a GPU test); None takes float64 numpy sums of the restated terms."""
    B, _, P = x.shape
    k0 = constants(oracle, rows, A, 0, np.zeros((B, 3, A)), P)  # g, g0, x0 do not depend on the sums
    L, c = logs_and_c(oracle, x, k0)
    xl, xc = pass1_terms(x, L, c)
    own = np.zeros((B, 3, A))
    own[:, 0] = x.astype(np.float64).sum(axis=2)
    if norm:
        own[:, 1], own[:, 2] = xl.sum(axis=2), xc.sum(axis=2)
    k = constants(oracle, rows, A, norm, own if sums is None else sums, P)
    t = terms(x, L, c, k, A)
    out = summary(t, A, k["dead"])
    out.update(t=t, sums=own, xl=xl, xc=xc, consts=k)
    return out
