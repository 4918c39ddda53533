"""The portable float32 restatement of smc_gbm_greeks' [B][26] block: the table of include/spectralmc_hip.h operation by
operation in numpy, on given terminal values and their logs.  Pure numpy and the oracle: importable without a GPU.
tests/test_gpu_greeks.py holds greeks_kernel to it (bit for bit where the kernel promises it, within sum-order bounds
elsewhere); tests/test_greeks_reference.py holds it to the independent float64 reference of
tests/helpers/greeks_reference.py.

In f32 the expectation follows the header's formulas in numpy float32 with the portable exp (oracle_exp2) and log
(oracle_log_pos); the sums are float64 in numpy's pairwise order, not the kernel's: hence the P 2^-52 bounds."""

from __future__ import annotations

import numpy as np

import oracle as _oracle


def log_pos_f32(q: np.ndarray) -> np.ndarray:
    fn = _oracle.oracle.lib().oracle_log_pos
    return np.array([fn(v) for v in q.ravel().tolist()], dtype=np.float32).reshape(q.shape)


def exp_any_f32(x: np.ndarray) -> np.ndarray:
    exp2 = _oracle.oracle.lib().oracle_exp2
    f32 = np.float32
    return np.array([exp2(float(f32(v) * f32(1.44269502))) for v in x], dtype=f32)


def terms(c: np.ndarray, term: np.ndarray, norm: int, sumx: np.ndarray, sumxl: np.ndarray | None,
           L: np.ndarray) -> dict[str, np.ndarray]:
    """The header's table on terminal values term [B,P] and their logs L [B,P] (both in the sim dtype): the ten
    per-path terms [10,B,P] in the sim dtype.  Every constant is taken in float64 from the contract row (and, under
    NORMALIZE, from sumx and sumxl) and rounded to the sim dtype; every per-path operation is rounded to it."""
    real = term.dtype.type
    P = term.shape[1]
    X0, K64, Tm, r, d, v = (c[:, i] for i in range(6))
    Tr = Tm.astype(real)
    if real is np.float32:
        F = X0.astype(real) * exp_any_f32((r - d).astype(real) * Tr)
        df = exp_any_f32((-r).astype(real) * Tr)
    else:
        F = X0 * np.exp((r - d) * Tm)
        df = np.exp(-r * Tm)
    K = K64.astype(real)
    s = F / (sumx / P).astype(real) if norm else np.ones(len(c), dtype=real)
    mu = r - d - 0.5 * v * v
    with np.errstate(divide="ignore", invalid="ignore"):
        ix0 = (1.0 / X0).astype(real)
        cv = np.where(v == 0, 0.0, 1.0 / v).astype(real)
        cT = np.where(Tm == 0, 0.0, 1.0 / (2.0 * Tm)).astype(real)
        crho = df * (Tr * K)
        rr = r.astype(real)
        if norm:
            lbar = sumxl / sumx
            av = np.where(v == 0, 0.0, -lbar / v).astype(real)
            aT = np.where(Tm == 0, r - d, -lbar / (2.0 * Tm) + (r - d)).astype(real)
        else:
            av = np.where(v == 0, 0.0, -mu * Tm / v - v * Tm).astype(real)
            aT = (mu / 2.0).astype(real)
    col = lambda a: a[:, None]  # noqa: E731
    zero = real(0)
    xs = term * col(s)
    dp, dc = col(K) - xs, xs - col(K)
    ip, ic = dp > zero, dc > zero
    put = col(df) * np.where(ip, dp, zero)
    call = col(df) * np.where(ic, dc, zero)
    w = col(df) * xs
    hv = L * col(cv) + col(av)
    hT = L * col(cT) + col(aT)
    wd, wv, wt = w * col(ix0), w * hv, w * hT
    crho_b = np.broadcast_to(col(crho), xs.shape)
    t = np.stack([np.where(ip, -wd, zero), np.where(ic, wd, zero),
                  np.where(ip, -wv, zero), np.where(ic, wv, zero),
                  np.where(ip, -crho_b, zero), np.where(ic, crho_b, zero),
                  col(rr) * put + np.where(ip, wt, zero), col(rr) * call - np.where(ic, wt, zero),
                  put, call])
    assert t.dtype == term.dtype and xs.dtype == term.dtype and hv.dtype == term.dtype
    return {"t": t, "xs": xs, "K": K, "crho": crho.astype(np.float64), "df": df.astype(np.float64),
            "F": F.astype(np.float64)}


def summary(t: np.ndarray, c: np.ndarray) -> dict[str, np.ndarray]:
    """From the terms [10,B,P]: the 24 columns 0..23 (float64 sums) and, per mean column 0..9 and price column,
    the sum-order bound P 2^-52 sum|term| / P and the ratio (mean|term|)^2 / var of the standard-error bound."""
    P = t.shape[2]
    t64 = t.astype(np.float64)
    s1, s2, sa = t64.sum(axis=2), (t64 * t64).sum(axis=2), np.abs(t64).sum(axis=2)   # [10,B]
    m = s1 / P
    D = np.maximum(s2 - P * m * m, 0.0)
    se = np.sqrt(D / (P - 1) / P) if P > 1 else np.zeros_like(m)
    bound = P * 2.0 ** -52 * sa / P
    den = c[:, 5] * c[:, 2] * c[:, 0] * c[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = lambda a: np.where(c[:, 5] * c[:, 2] == 0, 0.0, a / den)  # noqa: E731
        cols = np.stack([*m[:8], g(m[2]), g(m[3]), *se[:8], g(se[2]), g(se[3]), m[8], m[9], se[8], se[9]], axis=1)
        gb = np.stack([*bound[:8], g(bound[2]) + 2.0 ** -52 * np.abs(g(m[2])), g(bound[3]) + 2.0 ** -52 * np.abs(g(m[3]))])
        rho = np.square(sa / P) / (D / P)   # inf where every term is the same: see check_stderr
    # the term order of the 12 mean-and-error pairs of the block: columns (i, 10 + i) for i < 10, then (20, 22), (21, 23)
    return {"cols": cols, "bound": gb, "dD": P * 2.0 ** -52 * (s2 + 2 * sa * sa / P), "D": D, "rho": rho,
            "price_bound": bound[8:10]}


def check_stderr(got: np.ndarray, want: np.ndarray, summ: dict[str, np.ndarray], term: int, P: int, what: str,
                  scale: np.ndarray | None = None) -> None:
    """test_gpu_price's derivation for D = sum v^2 - P m^2 with e = P 2^-52: sum v^2 moves by e sum v^2 and P m^2
    by 2 e (sum |v|)^2 / P, so D by e (1 + 3 rho) D with rho = (mean |v|)^2 / var (m^2 / var for a term of one
    sign), halved by the square root: within 8 e max(1, rho / 2) relative.  Where D is not above four times that
    absolute movement dD (every path gives the same term, so D is rounding noise), only
    |sqrt(a) - sqrt(b)| <= sqrt(|a - b|) holds: within sqrt(dD / ((P - 1) P))."""
    e = P * 2.0 ** -52
    k = 1.0 if scale is None else scale
    D, dD, rho = summ["D"][term], summ["dD"][term], summ["rho"][term]
    flat = D <= 4 * dD
    with np.errstate(invalid="ignore"):
        tol = np.where(flat, np.sqrt(dD / max(P - 1, 1) / P) * k, 8 * e * np.maximum(1.0, rho / 2) * np.abs(want))
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / tol)
    print(f"{what} stderr: max share of its bound {share.max():.3f} ({int(flat.sum())} flat)")
    assert np.all(err <= tol), (what, int(np.argmax(share)))


def block(c: np.ndarray, term: np.ndarray, L: np.ndarray, norm: int, sumx: np.ndarray) -> np.ndarray:
    """The [B, 26] block from terminal values term [B, P], their logs L and the terminal sums sumx, with Lbar from
    the restatement's own float64 sum of the rounded products x L."""
    sumxl = (term * L).astype(np.float64).sum(axis=1)
    s = summary(terms(c, term, norm, sumx, sumxl, L)["t"], c)
    return np.concatenate([s["cols"], sumx[:, None], (sumxl if norm else np.zeros_like(sumxl))[:, None]], axis=1)


def block_f32(c: np.ndarray, T: int, P: int, seed: int, ordinal0: int, norm: int) -> np.ndarray:
    """The portable f32 block on the oracle's kernel-mode terminal values (the kernel's own streams and sum order)."""
    _oracle.build()
    _, term, rs = _oracle.kernel_paths(c, T, P, seed, ordinal0, 0)
    L = log_pos_f32(term / c[:, 0].astype(np.float32)[:, None])
    return block(c, term, L, norm, rs[:, -1].copy())


def block_f64(c: np.ndarray, T: int, P: int, seed: int, ordinal0: int, norm: int) -> np.ndarray:
    """The same formulas in float64 on the oracle's f64 paths, numpy's log."""
    _oracle.build()
    _, term, rs = _oracle.gbm_paths(c, T, P, seed, ordinal0, 0, dtype="float64")
    return block(c, term, np.log(term / c[:, 0][:, None]), norm, rs[:, -1].copy())
