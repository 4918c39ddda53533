"""An independent float64 reference of the path-dependent basket pricer (basket_path_kernel, smc_basket_price_paths),
with an a-priori bound on how far the f32 kernel may lie from it.  numpy only.

It stands on tests/helpers/basket_reference.py and tests/helpers/basket_general_reference.py (read those docstrings
first) and imports from them, unchanged: the drivers (stream words, Box-Muller), paths(..., L=...) with its
per-element relative bound of every row [B, A, T, P], the factor of the caller's matrix, scaled, _payoff and the
bound of the weighted sum.  From tests/helpers/gbm_reference.py it takes f32_error, mean_and_stderr and count_ok, and
the treatment of a knocked flag (_flips, restated below because that one reads a lower barrier <= 0 as "off", which
a spread's level does not allow).  It shares with the kernel only the stream words and the documented meaning of
include/spectralmc_hip.h: no f32 arithmetic, no Banachiewicz loop, no sweeps.

The model
---------
Rows x_it(p) of asset i, date t = 0 .. T - 1 (the T grid points; X0 is not a date), path p.  Under RAW xs = x.  Under
NORMALIZE xs_it = x_it F_it / (rowsum_it / P) with F_it = X0_i e^{(r - d_i) tau_t}, tau_t = (t + 1) T_m / T.  Then
    b_t = sum_i w_i xs_it,   m_t = min_i xs_it  (unweighted),
    avg = (1 / T) sum_t b_t,   mxb = max_t b_t,   mnb = min_t b_t,
    ko = any_t (b_t <= lower or b_t >= upper),   wko = any_t (m_t <= worst_lower),
and the 25 columns are the means of the ten payoffs df max(+-(K - u), 0) (Asian on avg; knock-out on b_{T-1} unless
ko; lookback put on mnb and call on mxb; worst-of on m_{T-1} unless wko; European on b_{T-1}), their standard errors,
and the means of avg, ko, wko, mxb, mnb.

The bound
---------
Derived, not fitted.  Inputs: the reference's own values, U = 2^-24, and what paths(), forwards' formula and scaled()
already carry.
* Row sums: basket_reference.terminal_sums' expression for every row (3 f32 roundings in the lane's partial sum, f64
  after that).
* Forwards: exp_any(f32(g) f32(tau)) as basket_reference.forwards charges it, with tau_t in place of T.
* Scales and scaled rows: basket_reference.scaled on the rows laid out as [B, A T, P]: each row is a "terminal row"
  with its own sum and forward.
* b_t: basket_general_reference.weighted (at most A + 1 roundings per term on magnitudes sum |w| (|xs| + delta)).
  m_t: 1-Lipschitz in the largest delta_xs of the row.
* avg: the running sum ((0 + b_0) + b_1) + ... has T - 1 roundings after the exact 0 + b_0, the division one more
  (f32(T) is exact): delta_avg = [sum_t delta_b_t + ((1 + U)^(T + 1) - 1) sum_t (|b_t| + delta_b_t)] / T, charged
  with T + 1 roundings.  mxb, mnb: 1-Lipschitz in the largest delta_b_t of the path.
* A knocked flag can differ from the reference's only on a path where some row lies within delta + |f32(bar) - bar|
  of a barrier and no row is surely outside (the worst flag is an "or" over assets and dates: each element with its
  own delta); such a path may carry its whole payoff (v + delta_v) or nothing.  The
  share columns move by the number of such paths over P.  count_ok (at most max(2, P / 256) such paths per contract
  and per flag) is the condition on the barriers a test may use.
* Payoffs, means, standard errors: _payoff and gbm_reference.mean_and_stderr (which take absolute values where a
  spread makes a level negative).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.helpers import basket_general_reference as gr
from tests.helpers import basket_reference as br
from tests.helpers.basket_reference import U, _exp_err, _payoff, compose, drivers, fields, paths, stream_words
from tests.helpers.gbm_reference import count_ok, f32_error, mean_and_stderr  # noqa: F401  (count_ok: for the tests)

COLS = 25
BLOCK = br.BLOCK


def row_forwards(rows: np.ndarray, A: int, T: int) -> tuple[np.ndarray, np.ndarray]:
    """(F [B, A, T], its relative bound): the forward of asset i at date t, tau_t = (t + 1) T_m / T."""
    _, Tm, r, _, X0, d, _ = fields(rows, A)
    tau = Tm[:, None] * (np.arange(1, T + 1) / T)[None, :]
    tau[:, -1] = Tm
    g = (r[:, None] - d)[:, :, None] * tau[:, None, :]
    return X0[:, :, None] * np.exp(g), compose(U, _exp_err(g), U)


def row_sums(x: np.ndarray, rel: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(rowsum, bound) [B, A, T] of rows [B, A, T, P]: basket_reference.terminal_sums' expression per row."""
    dx = x * rel
    tot = x.sum(axis=-1)
    return tot, dx.sum(axis=-1) + 3 * U * (x + dx).sum(axis=-1) + x.shape[-1] * 2.0 ** -52 * tot


def scaled_rows(rows: np.ndarray, A: int, x: np.ndarray, rel: np.ndarray, normalize: bool, *,
                terminal_scale: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(xs, delta_xs [B, A, T, P], rowsum, its bound [B, A, T]).  Wrong reading terminal_scale: the last row's scale
    applied to every row."""
    B, _, T, P = x.shape
    tot, tot_bound = row_sums(x, rel)
    F, eF = row_forwards(rows, A, T)
    if terminal_scale:
        tot_s, bound_s, F, eF = (np.repeat(a[:, :, -1:], T, axis=2) for a in (tot, tot_bound, F, eF))
    else:
        tot_s, bound_s = tot, tot_bound
    flat = lambda a: a.reshape(B, A * T, *a.shape[3:])  # noqa: E731
    xs, dxs = br.scaled(flat(x), flat(rel), flat(tot_s), flat(bound_s), normalize, flat(F), flat(eF))
    return xs.reshape(x.shape), dxs.reshape(x.shape), tot, tot_bound


def levels(xs: np.ndarray, dxs: np.ndarray, w: np.ndarray, *,
           weighted_min: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(b, delta_b, m, delta_m) [B, T, P] of scaled rows [B, A, T, P].  Wrong reading weighted_min: m over w_i xs_i."""
    B, A, T, P = xs.shape
    b, db = gr.weighted(xs.reshape(B, A, T * P), dxs.reshape(B, A, T * P), w)
    m = (w[:, :, None, None] * xs).min(axis=1) if weighted_min else xs.min(axis=1)
    return b.reshape(B, T, P), db.reshape(B, T, P), m, dxs.max(axis=1)


def worst_flags(xs: np.ndarray, dxs: np.ndarray, worst_lower: np.ndarray, strict: bool = False, *,
                x0: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(knocked [B, P], in doubt [B, P]) of m_t <= worst_lower at any date.  min_i xs_it <= bar exactly when some
    asset's value is, so the flag is flips' over every (asset, date) with that element's own bound: the assets of a
    contract may differ by decades, and the largest delta of the row says nothing about the smallest value.  x0
    [B, A] (wrong reading): X0 monitored as a date of its own."""
    B, A, T, P = xs.shape
    lev, dlev = xs.reshape(B, A * T, P), dxs.reshape(B, A * T, P)
    if x0 is not None:
        lev = np.concatenate([np.broadcast_to(x0[:, :, None], (B, A, P)), lev], axis=1)
        dlev = np.concatenate([np.zeros((B, A, P)), dlev], axis=1)
    return flips(lev, dlev, worst_lower, np.full(B, np.inf), strict)


def flips(level: np.ndarray, dlevel: np.ndarray, lower: np.ndarray, upper: np.ndarray,
          strict: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """(knocked [B, P], in doubt [B, P]) of levels [B, T, P] against barriers lower, upper [B]; -inf / +inf switch a
    side off.  gbm_reference._flips' treatment: a row outside may be inside for the kernel if it is outside by less
    than delta + beta, a row inside may be outside if it is inside by at most that; a path is in doubt if any row may
    flip and no row is surely outside.  Wrong reading strict: < and > for <= and >=."""
    lo, up = lower[:, None, None], upper[:, None, None]
    bl, bu = f32_error(lower)[:, None, None], f32_error(upper)[:, None, None]
    with np.errstate(invalid="ignore"):
        out_lo = (level < lo) if strict else (level <= lo)
        out_up = (level > up) if strict else (level >= up)
        gap_lo, gap_up = level - lo, up - level  # +inf where the side is off
    flip = np.where(out_lo, -gap_lo < dlevel + bl, gap_lo <= dlevel + bl) | \
        np.where(out_up, -gap_up < dlevel + bu, gap_up <= dlevel + bu)
    sure = ((out_lo & ~(-gap_lo < dlevel + bl)) | (out_up & ~(-gap_up < dlevel + bu))).any(axis=1)
    return (out_lo | out_up).any(axis=1), flip.any(axis=1) & ~sure


def default_barriers(rows: np.ndarray, A: int, w: np.ndarray, C: np.ndarray, sigmas: float = 1.0,
                     worst_sigmas: float = 1.5) -> np.ndarray:
    """[B, 3] (lower, upper, worst_lower): about one sigma sqrt(T) either side of the basket forward Fb = sum_i w_i F_i,
    the worst barrier 1.5 sigma sqrt(T) below the lowest forward.  The basket's sigma is that of its first-order
    lognormal: sigma^2 = sum_ij s_i s_j C_ij v_i v_j with s_i = w_i F_i / sum_k |w_k| F_k (signed, so a spread's forward,
    which may be near zero, is measured against sum |w| F); the worst barrier takes the largest v_i."""
    _, Tm, _, _, _, _, v = fields(rows, A)
    F = br.forwards(rows, A)[0]
    Fb, mag = (w * F).sum(axis=1), (np.abs(w) * F).sum(axis=1)
    sv = (w * F / mag[:, None]) * v
    s = np.sqrt(np.einsum("bi,bij,bj->b", sv, C, sv) * Tm)
    return np.stack([Fb - mag * (1.0 - np.exp(-sigmas * s)), Fb + mag * np.expm1(sigmas * s),
                     F.min(axis=1) * np.exp(-worst_sigmas * v.max(axis=1) * np.sqrt(Tm))], axis=1)


@dataclass
class PathRef:
    tot: np.ndarray         # [B, A] terminal sums
    tot_bound: np.ndarray
    cols: np.ndarray        # [B, 25]
    cols_bound: np.ndarray
    doubt: np.ndarray       # [B, 2] paths whose basket / worst knocked flag the bound leaves open
    b: np.ndarray           # [B, T, P] basket levels (the tests place barriers on them)
    db: np.ndarray


def path_columns(rows: np.ndarray, A: int, b: np.ndarray, db: np.ndarray, m: np.ndarray, dm: np.ndarray,
                 bars: np.ndarray | None, w: np.ndarray, *, wl: np.ndarray | None = None, dwl: np.ndarray | None = None,
                 strict: bool = False, with_x0: bool = False,
                 divide_by: int | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(columns [B, 25], their bounds, [B, 2] flags in doubt) from the levels [B, T, P]; wl, dwl [B, A, T, P]: the
    values the worst flag looks at (default: m itself with dm).  Wrong readings: strict barrier comparisons; with_x0:
    X0 monitored as a date of its own; divide_by: the average's divisor."""
    K = fields(rows, A)[0]
    assert np.all(K >= 0.0), "the payoff bound charges U K for the rounding of the strike"
    X0 = fields(rows, A)[4]
    B, T, P = b.shape
    _, _, df, edf = br.forwards(rows, A)
    bars = np.tile([-np.inf, np.inf, -np.inf], (B, 1)) if bars is None else np.asarray(bars, dtype=np.float64)
    bm, dbm = b, db
    if wl is None:
        wl, dwl = m[:, None], dm[:, None]
    if with_x0:
        b0 = np.broadcast_to((w * X0).sum(axis=1)[:, None, None], (B, 1, P))
        bm, dbm = np.concatenate([b0, b], axis=1), np.concatenate([np.zeros((B, 1, P)), db], axis=1)
    n = bm.shape[1]
    div = n if divide_by is None else divide_by
    S, dS = bm.sum(axis=1), dbm.sum(axis=1)
    avg = S / div
    davg = (dS + ((1.0 + U) ** (n + 1) - 1.0) * (np.abs(bm) + dbm).sum(axis=1)) / div
    mxb, mnb, dext = bm.max(axis=1), bm.min(axis=1), dbm.max(axis=1)
    ko, ko_doubt = flips(bm, dbm, bars[:, 0], bars[:, 1], strict)
    x0 = None if not with_x0 else (X0 if wl.shape[1] == A else X0.min(axis=1, keepdims=True))
    wko, wko_doubt = worst_flags(wl, dwl, bars[:, 2], strict, x0=x0)
    Kc, dfc, edfc = K[:, None], df[:, None], edf[:, None]
    eur = [_payoff(sign, Kc, b[:, -1], db[:, -1], dfc, edfc) for sign in (1.0, -1.0)]
    wor = [_payoff(sign, Kc, m[:, -1], dm[:, -1], dfc, edfc) for sign in (1.0, -1.0)]

    def knocked(pay, flag, doubt):  # a path in doubt may be paid in full or not at all
        v, dv = pay
        return np.where(flag, 0.0, v), np.where(doubt, v + dv, np.where(flag, 0.0, dv))

    pays = [_payoff(1.0, Kc, avg, davg, dfc, edfc), _payoff(-1.0, Kc, avg, davg, dfc, edfc),
            knocked(eur[0], ko, ko_doubt), knocked(eur[1], ko, ko_doubt),
            _payoff(1.0, Kc, mnb, dext, dfc, edfc), _payoff(-1.0, Kc, mxb, dext, dfc, edfc),
            knocked(wor[0], wko, wko_doubt), knocked(wor[1], wko, wko_doubt), eur[0], eur[1]]
    cols, bound = np.zeros((B, COLS)), np.zeros((B, COLS))
    for k, (v, dv) in enumerate(pays):
        cols[:, k], bound[:, k], cols[:, 10 + k], bound[:, 10 + k] = mean_and_stderr(v, dv)
    for col, (v, dv) in ((20, (avg, davg)), (23, (mxb, dext)), (24, (mnb, dext))):
        cols[:, col], bound[:, col], _, _ = mean_and_stderr(v, dv)
    cols[:, 21], bound[:, 21] = ko.mean(axis=1), ko_doubt.sum(axis=1) / P
    cols[:, 22], bound[:, 22] = wko.mean(axis=1), wko_doubt.sum(axis=1) / P
    return cols, bound, np.stack([ko_doubt.sum(axis=1), wko_doubt.sum(axis=1)], axis=1)


def outputs(rows: np.ndarray, A: int, x: np.ndarray, rel: np.ndarray, w: np.ndarray, bars: np.ndarray | None,
            normalize: bool, *, strict: bool = False, with_x0: bool = False, terminal_scale: bool = False,
            weighted_min: bool = False, divide_by: int | None = None) -> PathRef:
    """Everything downstream of the rows (x, rel) [B, A, T, P]."""
    xs, dxs, tot, tot_bound = scaled_rows(rows, A, x, rel, normalize, terminal_scale=terminal_scale)
    b, db, m, dm = levels(xs, dxs, w, weighted_min=weighted_min)
    wv = w[:, :, None, None] if weighted_min else 1.0
    cols, bound, doubt = path_columns(rows, A, b, db, m, dm, bars, w, wl=wv * xs, dwl=np.abs(wv) * dxs, strict=strict,
                                      with_x0=with_x0, divide_by=divide_by)
    return PathRef(tot[:, :, -1], tot_bound[:, :, -1], cols, bound, doubt, b, db)


def simulate(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, *,
             corr: np.ndarray | None = None, eps: br.MathEps = br.PORTABLE) -> tuple[np.ndarray, np.ndarray]:
    """(x, rel) [B, A, T, P]: every row of every asset and its relative bound (basket_reference.paths with the factor
    of the caller's matrix).  Computed once per case and math; outputs(...) reads it and leaves it unchanged."""
    rows = np.asarray(rows, dtype=np.float64)
    L = gr.factors(rows, A, corr)
    xs, rels = [], []
    for b0 in range(0, rows.shape[0], BLOCK):
        blk = rows[b0:b0 + BLOCK]
        z, rad = drivers(stream_words(oracle, blk.shape[0], A, T, P, seed, ordinal0 + b0))
        x, rel = paths(blk, A, T, z[:, :A, :, :P], rad[:, :A, :, :P], eps, L=L[b0:b0 + BLOCK])
        xs.append(x)
        rels.append(rel)
    return np.concatenate(xs), np.concatenate(rels)


def reference(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, *,
              weights: np.ndarray | None = None, corr: np.ndarray | None = None, barriers: np.ndarray | None = None,
              normalize: bool = True, eps: br.MathEps = br.PORTABLE, **wrong) -> PathRef:
    """smc_basket_price_paths' outputs for these contracts, and their bounds.  weights [A] or [B, A] (None: 1 / A),
    corr [A, A] or [B, A, A] (None: each row's rho), barriers [B, 3] (None: all off)."""
    rows = np.asarray(rows, dtype=np.float64)
    x, rel = simulate(oracle, rows, A, T, P, seed, ordinal0, corr=corr, eps=eps)
    return outputs(rows, A, x, rel, weights_of(weights, rows.shape[0], A), barriers, normalize, **wrong)


def weights_of(weights: np.ndarray | None, B: int, A: int) -> np.ndarray:
    return np.full((B, A), 1.0 / A) if weights is None else np.broadcast_to(np.asarray(weights, dtype=np.float64), (B, A))
