"""The portable float32 restatements of smc_gbm_price's [B][8] block and smc_gbm_price_paths' [B][20] block, in
numpy on the oracle's kernel-mode paths (oracle.kernel_paths, wg = 512: the kernels' own streams and sum order).
Pure numpy and the oracle: importable without a GPU.  tests/test_gpu_price.py and tests/test_gpu_path_price.py hold
the kernels to them bit for bit where the kernels promise it; tests/test_gbm_reference.py holds them to the
independent float64 reference of tests/helpers/gbm_reference.py.

F, df, K, the scales s = F / f32(sum / P) and the payoffs are taken in numpy float32 with the portable exp
(oracle_exp2), the sums in float64 (numpy's pairwise order, not the kernels': hence the P 2^-52 bounds of the tests)."""

from __future__ import annotations

import functools

import numpy as np

f32 = np.float32


@functools.lru_cache(maxsize=None)
def contracts(n: int) -> np.ndarray:
    """n contract rows (X0, K, T, r, d, v) around the money, read-only: the batch of the pricing tests."""
    rng = np.random.default_rng(2026)
    rows = []
    for _ in range(n):
        x0 = rng.uniform(50, 150)
        k = x0 * rng.uniform(0.8, 1.25)
        rows.append([x0, k, rng.uniform(0.25, 2), rng.uniform(-0.02, 0.08), rng.uniform(0, 0.04),
                     rng.uniform(0.1, 0.6)])
    out = np.array(rows, dtype=np.float64)
    out.setflags(write=False)
    return out


def barriers(c: np.ndarray) -> np.ndarray:
    """[B, 2] (lower, upper): L = X0 exp(-v sqrt(T)), U = max(X0, F) exp(v sqrt(T))."""
    X0, Tm, v = c[:, 0], c[:, 2], c[:, 5]
    F = X0 * np.exp((c[:, 3] - c[:, 4]) * Tm)
    return np.stack([X0 * np.exp(-v * np.sqrt(Tm)), np.maximum(X0, F) * np.exp(v * np.sqrt(Tm))], axis=1)


def time_grid(c: np.ndarray, T: int) -> np.ndarray:
    """[B, T] f64: linspace(dt, T, T), last point exact."""
    return np.stack([np.linspace(Tm / T, Tm, T, dtype=np.float64) for Tm in c[:, 2]])


def stderr(s1: np.ndarray, s2: np.ndarray, P: int) -> np.ndarray:
    if P == 1:
        return np.zeros_like(s1)
    m = s1 / P
    return np.sqrt(np.maximum(s2 - P * m * m, 0.0) / (P - 1) / P)


def exp_any_f32(oracle, x: np.ndarray) -> np.ndarray:
    """The portable e^x of csrc/smc_math.h exp_any, element by element through oracle_exp2."""
    exp2 = oracle.oracle.lib().oracle_exp2
    flat = [exp2(float(f32(v) * f32(1.44269502))) for v in np.asarray(x).ravel()]
    return np.array(flat, dtype=f32).reshape(np.shape(x))


def price_block(xs: np.ndarray, K: np.ndarray, F: np.ndarray, df: np.ndarray, tsum: np.ndarray) -> dict[str, np.ndarray]:
    """The 8 columns (and m^2 / var of put and call, [B,2]) from xs [B,P], K, F, df [B] in the sim dtype."""
    P = xs.shape[1]
    zero = xs.dtype.type(0)
    put = (df[:, None] * np.maximum(K[:, None] - xs, zero)).astype(np.float64)
    call = (df[:, None] * np.maximum(xs - K[:, None], zero)).astype(np.float64)
    sp, sc = put.sum(axis=1), call.sum(axis=1)
    sp2, sc2 = (put * put).sum(axis=1), (call * call).sum(axis=1)
    cols = np.stack([sp / P, sc / P, xs.astype(np.float64).sum(axis=1) / P, stderr(sp, sp2, P), stderr(sc, sc2, P),
                     (df * np.maximum(K - F, zero)).astype(np.float64),
                     (df * np.maximum(F - K, zero)).astype(np.float64), tsum], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = [np.square(s / P) / np.maximum(s2 / P - np.square(s / P), 1e-300) for s, s2 in ((sp, sp2), (sc, sc2))]
    return {"cols": cols, "m2_over_var": np.stack(ratio, axis=1), "F": F.astype(np.float64),
            "df": df.astype(np.float64)}


def price_f32(oracle, c: np.ndarray, T: int, P: int, seed: int, ordinal0: int, scheme: int,
              norm: int) -> dict[str, np.ndarray]:
    """smc_gbm_price's block for the contracts c in portable f32 math."""
    oracle.build()
    B = c.shape[0]
    _, term, rs = oracle.kernel_paths(c, T, P, seed, ordinal0, scheme)
    Tm = c[:, 2].astype(f32)
    F = c[:, 0].astype(f32) * exp_any_f32(oracle, (c[:, 3] - c[:, 4]).astype(f32) * Tm)
    df = exp_any_f32(oracle, (-c[:, 3]).astype(f32) * Tm)
    K = c[:, 1].astype(f32)
    tsum = rs[:, -1].copy()
    s = F / (tsum / P).astype(f32) if norm else np.ones(B, dtype=f32)
    xs = term * s[:, None]
    assert xs.dtype == f32 and F.dtype == f32 and df.dtype == f32
    return price_block(xs, K, F, df, tsum)


def path_block(xs: np.ndarray, K: np.ndarray, df: np.ndarray, lower: np.ndarray, upper: np.ndarray) -> dict[str, np.ndarray]:
    """The 20 columns (and m^2 / var of the 8 payoffs, [B, 8]) from the scaled rows xs [B, T, P] and K, df, the
    barriers [B], all in the sim dtype: the per-path state row by row in that dtype, the sums in float64."""
    B, T, P = xs.shape
    real = xs.dtype.type
    zero = real(0)
    a = np.zeros((B, P), dtype=xs.dtype)
    mx = np.full((B, P), -np.inf, dtype=xs.dtype)
    mn = np.full((B, P), np.inf, dtype=xs.dtype)
    ko = np.zeros((B, P), dtype=bool)
    for t in range(T):
        row = xs[:, t, :]
        a = a + row
        mx = np.maximum(mx, row)
        mn = np.minimum(mn, row)
        ko |= (row <= lower[:, None]) | (row >= upper[:, None])
    avg = a / real(T)
    last = xs[:, T - 1, :]
    assert avg.dtype == xs.dtype and K.dtype == xs.dtype and df.dtype == xs.dtype and lower.dtype == xs.dtype

    def pay(diff: np.ndarray) -> np.ndarray:
        v = df[:, None] * np.maximum(diff, zero)
        assert v.dtype == xs.dtype
        return v.astype(np.float64)

    Kc = K[:, None]
    put, call = pay(Kc - last), pay(last - Kc)
    pays = [pay(Kc - avg), pay(avg - Kc), np.where(ko, 0.0, put), np.where(ko, 0.0, call), pay(Kc - mn), pay(mx - Kc),
            put, call]
    s1 = np.stack([v.sum(axis=1) for v in pays], axis=1)
    s2 = np.stack([(v * v).sum(axis=1) for v in pays], axis=1)
    cols = np.empty((B, 20))
    cols[:, :8] = s1 / P
    cols[:, 8:16] = stderr(s1, s2, P)
    cols[:, 16] = avg.astype(np.float64).sum(axis=1) / P
    cols[:, 17] = ko.sum(axis=1) / P
    cols[:, 18] = mx.astype(np.float64).sum(axis=1) / P
    cols[:, 19] = mn.astype(np.float64).sum(axis=1) / P
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.square(s1 / P) / np.maximum(s2 / P - np.square(s1 / P), 1e-300)
    return {"cols": cols, "m2_over_var": rho}


def path_price_f32(oracle, c: np.ndarray, bars: np.ndarray, T: int, P: int, seed: int, ordinal0: int, scheme: int,
                   norm: int) -> dict[str, np.ndarray]:
    """smc_gbm_price_paths' block for the contracts c and barriers [B, 2] in portable f32 math."""
    oracle.build()
    B = c.shape[0]
    paths, _, rs = oracle.kernel_paths(c, T, P, seed, ordinal0, scheme, want_paths=True)
    Tm = c[:, 2].astype(f32)
    df = exp_any_f32(oracle, (-c[:, 3]).astype(f32) * Tm)
    K = c[:, 1].astype(f32)
    if norm:
        F = c[:, 0].astype(f32)[:, None] * exp_any_f32(oracle, (c[:, 3] - c[:, 4]).astype(f32)[:, None]
                                                       * time_grid(c, T).astype(f32))
        s = F / (rs / P).astype(f32)
        assert s.dtype == f32 and s.shape == (B, T)
        xs = paths * s[:, :, None]
    else:
        xs = paths
    assert xs.dtype == f32
    bars = np.asarray(bars).astype(f32)
    return path_block(xs, K, df, bars[:, 0], bars[:, 1])
