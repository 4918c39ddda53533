"""The portable float32 restatement of smc_gbm_greeks_paths' [B][40] block: the table of include/spectralmc_hip.h
statement by statement in numpy, on the oracle's kernel-mode rows (oracle.kernel_paths, wg = 512: the kernel's own
streams and row sums).  Pure numpy and the oracle: importable without a GPU.  Unlike the other restatements the sums
here run in the kernel's own order (per lane over its chunks and paths, the wave butterfly xor 32..1, waves 0..7),
so tests/test_gpu_path_greeks.py holds path_greeks_kernel to it bit for bit; tests/test_path_greeks_reference.py
holds it to the independent float64 reference of tests/helpers/path_greeks_reference.py."""

from __future__ import annotations

import numpy as np

import oracle as _oracle

from . import gbm_restate, greeks_restate

f32 = np.float32
THREADS, LANE_PATHS, WAVES = 512, 4, 8
CHUNK = THREADS * LANE_PATHS
PAYOFFS = ("asian_put", "asian_call", "lookback_put", "lookback_call")
GREEKS = ("delta", "vega", "rho", "theta")
COLS = 40


def kernel_sum(vals: np.ndarray) -> np.ndarray:
    """The sum of float64 vals [..., P] over P in the kernels' order: path p belongs to chunk p // 2048, lane
    (p % 2048) // 4; a lane adds its values chunk by chunk and path by path from 0.0; the 64 lanes of a wave go
    through the butterfly v += v[lane ^ off], off = 32 .. 1; wave 0's total takes waves 1..7 in order."""
    assert vals.dtype == np.float64
    P = vals.shape[-1]
    nch = -(-P // CHUNK)
    pad = np.zeros(vals.shape[:-1] + (nch * CHUNK,))  # a lane past P adds nothing: + 0.0 leaves a sum as it is
    pad[..., :P] = vals
    arr = pad.reshape(vals.shape[:-1] + (nch, THREADS, LANE_PATHS))
    lane = np.zeros(vals.shape[:-1] + (THREADS,))
    for c in range(nch):
        for j in range(LANE_PATHS):
            lane = lane + arr[..., c, :, j]
    w = lane.reshape(vals.shape[:-1] + (WAVES, 64))
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., idx ^ off]
    tot = np.zeros(vals.shape[:-1])
    for k in range(WAVES):
        tot = tot + w[..., k, 0]
    return tot


def block_from_rows(c: np.ndarray, x: np.ndarray, sumx: np.ndarray, norm: int) -> dict[str, np.ndarray]:
    """The [B, 40] block from the raw rows x [B, T, P] (f32), their kernel-order row sums sumx [B, T] (f64) and the
    contracts c [B, 6].  Also returns the row tables and sumxl."""
    B, T, P = x.shape
    assert x.dtype == f32
    X0, K64, Tm, r, d, v = (c[:, i] for i in range(6))
    col = lambda a: a[:, None]  # noqa: E731
    tau = gbm_restate.time_grid(c, T)                                  # [B, T] f64, row_forward's grid
    fr = np.broadcast_to((np.arange(T) + 1.0) / T, (B, T))
    mu = r - d - 0.5 * v * v
    x0 = X0.astype(f32)
    L = greeks_restate.log_pos_f32(x / x0[:, None, None])              # L_t [B, T, P] f32
    Tr = Tm.astype(f32)
    K = K64.astype(f32)
    df = gbm_restate.exp_any_f32(_oracle, (-r).astype(f32) * Tr)
    with np.errstate(divide="ignore", invalid="ignore"):
        ix0 = (1.0 / X0).astype(f32)
        cv = np.where(v == 0, 0.0, 1.0 / v).astype(f32)
        cT = np.where(Tm == 0, 0.0, 1.0 / (2.0 * Tm)).astype(f32)
        rr = r.astype(f32)
        tr = tau.astype(f32)
        if norm:
            F = x0[:, None] * gbm_restate.exp_any_f32(_oracle, (r - d).astype(f32)[:, None] * tau.astype(f32))
            s = F / (sumx / P).astype(f32)
            sumxl = kernel_sum((x * L).astype(np.float64))             # [B, T]: the product in f32, added singly
            lbar = sumxl / sumx
            av = np.where(col(v) == 0, 0.0, -lbar / col(v)).astype(f32)
            aT = np.where(col(Tm) == 0, col(r - d) * fr, -lbar / (2.0 * col(Tm)) + col(r - d) * fr).astype(f32)
        else:
            s = np.ones((B, T), dtype=f32)
            sumxl = np.zeros((B, T))
            av = np.where(col(v) == 0, 0.0, -col(mu) * tau / col(v) - col(v) * tau).astype(f32)
            aT = (col(mu) / 2.0 * fr).astype(f32)
    assert s.dtype == f32 and av.dtype == f32 and aT.dtype == f32 and tr.dtype == f32

    zero = f32(0)
    sa = np.zeros((B, P), f32)
    sv, sT, sr = sa.copy(), sa.copy(), sa.copy()
    mx = np.full((B, P), -np.inf, f32)
    mn = np.full((B, P), np.inf, f32)
    Lmx, Lmn = sa.copy(), sa.copy()
    tmx = np.zeros((B, P), dtype=np.int64)
    tmn = tmx.copy()
    for t in range(T):
        Lt = L[:, t, :]
        xs = x[:, t, :] * s[:, t, None] if norm else x[:, t, :]
        hv = Lt * col(cv) + av[:, t, None]
        hT = Lt * col(cT) + aT[:, t, None]
        sa = sa + xs
        sv = sv + xs * hv
        sT = sT + xs * hT
        sr = sr + xs * tr[:, t, None]
        up = xs > mx                                                   # strict: the first row wins a tie
        mx, Lmx, tmx = np.where(up, xs, mx), np.where(up, Lt, Lmx), np.where(up, t, tmx)
        dn = xs < mn
        mn, Lmn, tmn = np.where(dn, xs, mn), np.where(dn, Lt, Lmn), np.where(dn, t, tmn)
    steps = f32(T)
    take = lambda tab, at: np.take_along_axis(tab, at, axis=1)  # noqa: E731
    under = {
        "asian": (sa / steps, sv / steps, sT / steps, sr / steps),
        "max": (mx, mx * (Lmx * col(cv) + take(av, tmx)), mx * (Lmx * col(cT) + take(aT, tmx)), mx * take(tr, tmx)),
        "min": (mn, mn * (Lmn * col(cv) + take(av, tmn)), mn * (Lmn * col(cT) + take(aT, tmn)), mn * take(tr, tmn)),
    }

    def terms(is_put: bool, u: np.ndarray, gv: np.ndarray, gT: np.ndarray, gr: np.ndarray) -> list[np.ndarray]:
        diff = col(K) - u if is_put else u - col(K)
        inm = diff > zero
        pay = col(df) * np.where(inm, diff, zero)
        wd, wv, wr, wT = (col(df) * u) * col(ix0), col(df) * gv, col(df) * gr, col(df) * gT
        if is_put:
            out = [np.where(inm, -wd, zero), np.where(inm, -wv, zero), -(col(Tr) * pay) - np.where(inm, wr, zero),
                   col(rr) * pay + np.where(inm, wT, zero), pay]
        else:
            out = [np.where(inm, wd, zero), np.where(inm, wv, zero), -(col(Tr) * pay) + np.where(inm, wr, zero),
                   col(rr) * pay - np.where(inm, wT, zero), pay]
        assert all(o.dtype == f32 for o in out)
        return out

    per_payoff = [terms(True, *under["asian"]), terms(False, *under["asian"]), terms(True, *under["min"]),
                  terms(False, *under["max"])]
    cols = np.empty((B, COLS))
    n = float(P)
    for q, tq in enumerate(per_payoff):
        for g, t in enumerate(tq):
            t64 = t.astype(np.float64)
            s1, s2 = kernel_sum(t64), kernel_sum(t64 * t64)
            m = s1 / n
            se = np.sqrt(np.maximum(s2 - n * m * m, 0.0) / (n - 1.0) / n) if P > 1 else np.zeros(B)
            if g < 4:
                cols[:, 4 * g + q], cols[:, 16 + 4 * g + q] = m, se
            else:
                cols[:, 32 + q], cols[:, 36 + q] = m, se
    return {"cols": cols, "scales": s, "tr": tr, "av": av, "aT": aT, "sumxl": sumxl}


def block_f32(c: np.ndarray, T: int, P: int, seed: int, ordinal0: int, norm: int) -> np.ndarray:
    """smc_gbm_greeks_paths' block for the contracts c in portable f32 math, log-Euler."""
    _oracle.build()
    paths, _, rs = _oracle.kernel_paths(c, T, P, seed, ordinal0, 0, want_paths=True)
    return block_from_rows(c, paths, rs, norm)["cols"]
