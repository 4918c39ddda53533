"""An independent float64 reference of the pathwise Greeks of the Asian and lookback basket options
(smc_basket_greeks_paths, basket_path_greeks_kernel of csrc/basket.hip), with an a-priori bound on how far the f32
kernel may lie from it, in portable and in SMC_MATH_HW math.  numpy only.

What it shares with the kernel: the stream words and drivers (basket_reference.stream_words, drivers), the rows with
their per-element relative bounds (basket_reference.paths(..., L=) on numpy.linalg.cholesky's factor of the caller's
matrix), basket_path_reference's row sums, forwards, scales and levels, basket_reference's payoff,
gbm_reference.mean_and_stderr, and the documented meaning of the 16A + 24 columns (include/spectralmc_hip.h).  What
it does not share: any arithmetic of the kernel.  No log of a simulated value enters a derivative: the Brownian terms
come from the driver sums.

The model
---------
Asset i, row t (0-based) of T rows: tau_t = (t + 1) T_m / T, fr_t = (t + 1) / T, W_it = sqrt(dt) sum_{s <= t} (Lc z_s)_i,
x_it = X0_i exp(mu_i tau_t + v_i W_it), mu_i = r - d_i - v_i^2 / 2.  W does not depend on X0_i, v_i, r or T_m, so
    d ln x_it / d v_i = W_it - v_i tau_t      d ln x_it / d T = mu_i fr_t + v_i W_it / (2 T_m)   (every date moves with T)
    d ln x_it / d X0_i = 1 / X0_i             d ln x_it / d r = tau_t
and asset i's rows do not move with X0_j, v_j for j != i.  RAW: xs = x.  NORMALIZE: xs_it = x_it F_it / mean_p(x_it):
for v_i and T the derivative of ln xs_it is that of ln x_it less its x_it-weighted mean over the paths, plus that of
ln F_it ((r - d_i) fr_t for T, 0 for v_i); for X0_i and r, x, F and the mean move alike.
b_t = sum_i w_i xs_it.  Underlyings: the Asian average u = mean_t b_t, the lookback put's min_t b_t and call's
max_t b_t, taken at the row t* of the extreme (the first one on a tie):
    du / dX0_i = (1 / T) sum_t w_i xs_it / X0_i          or  w_i xs_it* / X0_i
    du / dv_i  = (1 / T) sum_t w_i xs_it d ln xs_it/dv_i  or  the t* term
    du / dT    = (1 / T) sum_t sum_i w_i xs_it d ln xs_it/dT,   du / dr = (1 / T) sum_t b_t tau_t    or the t* terms.
With df = e^{-r T}, put = df max(K - u, 0), call = df max(u - K, 0), ip = 1{K > u}, ic = 1{u > K}:
    delta_i  -+ 1{.} df du/dX0_i          vega_i  -+ 1{.} df du/dv_i
    rho      -T put - ip df du/dr,  -T call + ic df du/dr
    theta    = -dV/dT:  r put + ip df du/dT,  r call - ic df du/dT.
Greek kinds g = delta_0 .. delta_{A-1}, vega_0 .. vega_{A-1}, rho, theta (G = 2A + 2); payoffs q = Asian put, Asian
call, lookback put, lookback call.  Column 4 g + q is the mean, 4 G + 4 g + q its standard error, 8 G + q the price,
8 G + 4 + q its standard error.  Conventions of the header: v_i == 0 gives d ln xs_it / d v_i = 0.

The bound
---------
Nothing is fitted to the kernel.  Inputs: the reference's own values, U = 2^-24, what paths(), scaled_rows() and
levels() carry, and greeks_reference's LogEps for the log.  path_greeks_reference's prod and add rules (with u = U)
do the propagation, and its two kinds of doubt are treated as there.
* L_it = log(fl(x_it / fl(X0_i))) by greeks_reference.log_bound.
* Row constants: tau_t an f64 value rounded once (2 U charged: the f64 grid point carries two roundings of its own);
  cv_i, cT, ix0_i, w_i rounded once; av_it, aT_it f64 values rounded once.  Under NORMALIZE Lbar_it = sumxl_it /
  sumx_it: sumxl by prod over the paths plus the f64 summation, sumx by basket_path_reference.row_sums.
* hv = fl(fl(L cv) + av), hT = fl(fl(L cT) + aT) by prod and add; wx = fl(w xs) by prod; a running sum of n terms
  and the division by steps: n + 1 roundings against the sum of the absolute terms (basket_path_reference's rule for
  avg); rowT, a running sum of A products: A roundings.
* df times a derivative by prod; put and call by basket_reference._payoff; T put, r put by prod; the sums by add.
* A path with |u - K| <= du + |fl(K) - K| may have either indicator: each indicator term of it carries its whole live
  value, plus that value's bound, as error (doubt_ind counts such paths over the payoff families).
* The lookback row: every row whose level lies within the two rows' bounds of the extreme is a candidate; the path is
  charged the largest distance of a candidate's term (plus its bound) from the reference's (doubt_arg counts the paths
  with more than one candidate).  A flat contract (every v_i == 0 with r == d_i, or T == 0) keeps every row on
  fl(X0_i) exactly in the kernel too: its rows tie exactly, the first row wins there as here, nothing is in doubt.
* Means and standard errors by gbm_reference.mean_and_stderr.

The keyword arguments of `greeks` listed in WRONG are wrong readings, for tests/test_basket_path_greeks_reference.py.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.helpers import basket_general_reference as gr
from tests.helpers import basket_path_reference as bp
from tests.helpers import basket_reference as br
from tests.helpers import greeks_reference as gk
from tests.helpers.basket_reference import U, fields
from tests.helpers.gbm_reference import count_ok, mean_and_stderr  # noqa: F401  (count_ok: for the tests)
from tests.helpers.path_greeks_reference import add, arg_ok, prod  # noqa: F401  (arg_ok: for the tests)

PAYOFFS = ("asian_put", "asian_call", "lookback_put", "lookback_call")
WRONG = ("no_lbar", "terminal_tau", "last_tie", "maturity_only", "vega_cross", "abs_w", "over_T1")
EPS = {"portable": br.PORTABLE, "hw": br.HW}


def cols(A: int) -> int:
    return 16 * A + 24


def kinds(A: int) -> int:
    return 2 * A + 2


def column(A: int, g: int, q: int, stderr: bool = False) -> int:
    """Greek kind g (delta_i: i, vega_i: A + i, rho: 2A, theta: 2A + 1, price: 2A + 2) of payoff q."""
    G = kinds(A)
    if g == G:
        return 8 * G + (4 if stderr else 0) + q
    return (4 * G if stderr else 0) + 4 * g + q


def mean_columns(A: int) -> list[int]:
    G = kinds(A)
    return list(range(4 * G)) + list(range(8 * G, 8 * G + 4))


def price_columns(A: int) -> list[int]:
    return list(range(16 * A + 16, 16 * A + 24))


@dataclass
class BasketPathGreeksRef:
    cols: np.ndarray       # [B, 16A + 24]
    bound: np.ndarray      # [B, 16A + 24]
    doubt_ind: np.ndarray  # [B] paths with an indicator the bound leaves open (Asian or lookback)
    doubt_arg: np.ndarray  # [B] paths whose row of the maximum or of the minimum the bound leaves open
    terms: np.ndarray      # [G + 1, 4, B, P] per-path terms (kind, payoff)


def _running(val, dval, axis, n_round):
    """(sum, bound) of a running f32 sum over `axis` with n_round roundings."""
    S, dS = val.sum(axis=axis), dval.sum(axis=axis)
    return S, dS + ((1.0 + U) ** n_round - 1.0) * (np.abs(val).sum(axis=axis) + dS)


def _terms(rows, A, sign, un, dun, wd, wv, wT, wr):
    """The G + 1 per-path terms of one payoff and their bounds.  un, dun [B, ...]: the underlying; wd, wv = (value,
    bound) [B, A, ...]: df du/dX0_i and df du/dv_i; wT, wr = (value, bound) [B, ...]: df du/dT and df du/dr."""
    K, Tm, r = fields(rows, A)[:3]
    _, _, df, edf = br.forwards(rows, A)
    ex = lambda a: np.asarray(a).reshape((-1,) + (1,) * (un.ndim - 1))  # noqa: E731
    pay, dpay = br._payoff(sign, ex(K), un, dun, ex(df), ex(edf))
    ind = sign * (ex(K) - un) > 0
    open_ = np.abs(un - ex(K)) <= dun + U * np.abs(ex(K))

    def gated(s, ds, sg, per_asset=False):
        i_, o_ = (ind[:, None], open_[:, None]) if per_asset else (ind, open_)
        return np.where(i_, sg * s, 0.0), np.where(o_, np.abs(s) + ds, np.where(i_, ds, 0.0))

    delta = gated(wd[0], wd[1], -sign, True)
    vega = gated(wv[0], wv[1], -sign, True)
    gr_, gT_ = gated(wr[0], wr[1], -sign), gated(wT[0], wT[1], sign)
    Tp, dTp = -ex(Tm) * pay, prod(ex(Tm), U * np.abs(ex(Tm)), pay, dpay, U)
    rp, drp = ex(r) * pay, prod(ex(r), U * np.abs(ex(r)), pay, dpay, U)
    out = [(delta[0][:, i], delta[1][:, i]) for i in range(A)] + [(vega[0][:, i], vega[1][:, i]) for i in range(A)]
    out.append((Tp + gr_[0], add(Tp, dTp, gr_[0], gr_[1], U)))
    out.append((rp + gT_[0], add(rp, drp, gT_[0], gT_[1], U)))
    out.append((pay, dpay))
    return out, open_


def greeks(rows: np.ndarray, A: int, T: int, z: np.ndarray, radius: np.ndarray, w: np.ndarray, Lf: np.ndarray,
           math: str = "portable", *, normalize: bool = True, **wrong: bool) -> BasketPathGreeksRef:
    """The 16A + 24 columns for contract rows [B, 3A + 4], drivers z, radius [B, A, T, P], weights w [B, A] and
    factors Lf [B, A, A], with bounds."""
    assert set(wrong) <= set(WRONG)
    wr_ = {k: bool(wrong.get(k, False)) for k in WRONG}
    rows = np.asarray(rows, dtype=np.float64)
    K, Tm, r, _, X0, d, v = fields(rows, A)
    B, _, _, P = z.shape
    G = kinds(A)
    leps = gk.LOGS[math]
    a2 = lambda a: np.asarray(a)[:, :, None, None]   # noqa: E731  [B, A] -> [B, A, 1, 1]
    rt = lambda a: np.asarray(a)[:, None, :, None]   # noqa: E731  [B, T] -> [B, 1, T, 1]
    x, rel = br.paths(rows, A, T, z, radius, EPS[math], L=Lf)
    fr = np.arange(1, T + 1, dtype=np.float64)[None, :] / T                      # [1, T]
    tau = Tm[:, None] * fr                                                        # [B, T]
    tau_h, fr_h = tau, np.broadcast_to(fr, tau.shape)
    if wr_["terminal_tau"]:
        tau_h, fr_h = np.broadcast_to(Tm[:, None], tau.shape), np.ones_like(tau)
    W = np.cumsum(np.sqrt(Tm / T)[:, None, None, None] * np.einsum("bik,bktp->bitp", Lf, z), axis=2)
    mu = r[:, None] - d - v * v / 2
    Lg = a2(mu) * rt(tau) + a2(v) * W                                             # ln(x / X0), from the drivers
    live_v, live_T = a2(v != 0), (Tm != 0)[:, None, None, None]
    flat = (np.all(v == 0, axis=1) & np.all(r[:, None] == d, axis=1)) | (Tm == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        hv = np.where(live_v, W - a2(v) * rt(tau_h), 0.0)
        hT = np.where(live_T, a2(mu) * rt(fr_h) + a2(v) * W / (2 * Tm)[:, None, None, None], a2(mu / 2) * rt(fr_h))
        cv = np.where(v != 0, 1 / v, 0.0)
        cT = np.where(Tm != 0, 1 / (2 * Tm), 0.0)
    ix0 = 1 / X0
    last = (np.arange(T) == T - 1)[None, None, :, None]
    if wr_["maturity_only"]:
        hT = hT * last
    # the log the kernel takes
    eq = (1 + rel) * (1 + U) / (1 - U) - 1
    dL = gk.log_bound(np.exp(Lg), eq, leps)
    xs, dxs, sumx, dsumx = bp.scaled_rows(rows, A, x, rel, normalize)             # sums [B, A, T]
    rd = r[:, None] - d
    if normalize:
        xL = x * Lg
        sumxl = xL.sum(axis=3)
        dsumxl = prod(x, x * rel, Lg, dL, U).sum(axis=3) + P * 2.0 ** -52 * np.abs(xL).sum(axis=3)
        lbar = sumxl / sumx
        dlbar = (dsumxl + np.abs(lbar) * dsumx) / (sumx - dsumx)
        wmean = lambda a: ((x * a).sum(axis=3) / sumx)[:, :, :, None]             # noqa: E731
        if not wr_["no_lbar"]:
            hv = np.where(live_v, hv - wmean(hv), 0.0)
            hT = hT - wmean(hT)
        carry = a2(rd) * rt(fr_h)
        if wr_["maturity_only"]:
            carry = carry * last
        hT = np.where(live_T, hT + carry, carry)
        av = -lbar * cv[:, :, None]
        dav = dlbar * cv[:, :, None] * (1 + U) + U * np.abs(av)
        aT = -lbar * cT[:, None, None] + rd[:, :, None] * fr[:, None, :]
        daT = dlbar * cT[:, None, None] * (1 + U) + U * np.abs(aT)
    else:
        av = np.where(v[:, :, None] != 0, -mu[:, :, None] * tau[:, None, :] * cv[:, :, None] - v[:, :, None] * tau[:, None, :],
                      0.0)
        aT = (mu / 2)[:, :, None] * fr[:, None, :]
        dav, daT = 2 * U * np.abs(av), 2 * U * np.abs(aT)
    cT4 = cT[:, None, None, None]
    Lcv, LcT = Lg * a2(cv), Lg * cT4
    dhv = add(Lcv, prod(Lg, dL, a2(cv), a2(U * cv), U), av[..., None], dav[..., None], U)
    dhT = add(LcT, prod(Lg, dL, cT4, U * cT4, U), aT[..., None], daT[..., None], U)
    dhv = np.where(live_v, dhv, 0.0)                 # cv = av = 0 exactly: hv = fl(L 0 + 0) = 0
    if wr_["vega_cross"]:
        hv = np.roll(hv, 1, axis=1)
    wq = np.abs(w) if wr_["abs_w"] else w
    wx, dwx = a2(wq) * xs, prod(a2(wq), a2(U * np.abs(wq)), xs, dxs, U)           # [B, A, T, P]
    b, db, _, _ = bp.levels(xs, dxs, w)                                           # [B, T, P]
    pv = (wx * hv, prod(wx, dwx, hv, dhv, U))
    pT = (wx * hT, prod(wx, dwx, hT, dhT, U))
    rowT = _running(pT[0], pT[1], 1, A)                                           # [B, T, P]
    tau3, dtau3 = tau_h[:, :, None], 2 * U * np.abs(tau_h)[:, :, None]
    br_ = (b * tau3, prod(b, db, tau3, dtau3, U))
    _, _, df, edf = br.forwards(rows, A)
    df2, ddf2 = df[:, None], (df * edf)[:, None]
    df3, ddf3 = df[:, None, None], (df * edf)[:, None, None]
    df4, ddf4 = df[:, None, None, None], (df * edf)[:, None, None, None]
    n = T + 1 if wr_["over_T1"] else T

    def averaged(val, dval, axis):
        S, dS = _running(val, dval, axis, T + 1)
        return S / n, dS / n

    terms = np.zeros((G + 1, 4, B, P))
    dterms = np.zeros_like(terms)
    doubt_ind = np.zeros((B, P), dtype=bool)
    # the Asian payoffs
    ua, dua = averaged(b, db, 1)
    sd = averaged(wx, dwx, 2)                                                     # [B, A, P]
    ix3 = ix0[:, :, None]
    du0 = (sd[0] * ix3, prod(sd[0], sd[1], ix3, U * ix3, U))
    wd = (df3 * du0[0], prod(df3, ddf3, du0[0], du0[1], U))
    gv = averaged(pv[0], pv[1], 2)
    wv = (df3 * gv[0], prod(df3, ddf3, gv[0], gv[1], U))
    gT = averaged(rowT[0], rowT[1], 1)
    wT = (df2 * gT[0], prod(df2, ddf2, gT[0], gT[1], U))
    gR = averaged(br_[0], br_[1], 1)
    wr = (df2 * gR[0], prod(df2, ddf2, gR[0], gR[1], U))
    for q, sign in ((0, 1.0), (1, -1.0)):
        tq, open_ = _terms(rows, A, sign, ua, dua, wd, wv, wT, wr)
        doubt_ind |= open_
        for g, (val, dval) in enumerate(tq):
            terms[g, q], dterms[g, q] = val, dval
    # the lookback payoffs: the terms at every row, then the row of the extreme and its candidates
    t1 = (df4 * wx, prod(df4, ddf4, wx, dwx, U))
    ix4 = a2(ix0)
    wd_r = (t1[0] * ix4, prod(t1[0], t1[1], ix4, U * ix4, U))                     # [B, A, T, P]
    wv_r = (df4 * pv[0], prod(df4, ddf4, pv[0], pv[1], U))
    wT_r = (df3 * rowT[0], prod(df3, ddf3, rowT[0], rowT[1], U))                  # [B, T, P]
    wr_r = (df3 * br_[0], prod(df3, ddf3, br_[0], br_[1], U))
    doubt_arg = np.zeros((B, P), dtype=bool)
    for q, sign, take_max in ((2, 1.0, False), (3, -1.0, True)):
        key = b if take_max else -b
        at = (T - 1 - np.argmax(key[:, ::-1], axis=1)) if wr_["last_tie"] else np.argmax(key, axis=1)
        best = np.take_along_axis(key, at[:, None, :], axis=1)
        dbest = np.take_along_axis(db, at[:, None, :], axis=1)
        cand = np.where(flat[:, None, None], np.arange(T)[None, :, None] == at[:, None, :], best - key <= db + dbest)
        doubt_arg |= cand.sum(axis=1) > 1
        tq, open_ = _terms(rows, A, sign, b, db, wd_r, wv_r, wT_r, wr_r)
        doubt_ind |= np.take_along_axis(open_, at[:, None, :], axis=1)[:, 0]
        for g, (val, dval) in enumerate(tq):
            ref = np.take_along_axis(val, at[:, None, :], axis=1)
            terms[g, q] = ref[:, 0]
            dterms[g, q] = np.where(cand, np.abs(val - ref) + dval, 0.0).max(axis=1)
    out, bound = np.zeros((B, cols(A))), np.zeros((B, cols(A)))
    for g in range(G + 1):
        for q in range(4):
            m, s = column(A, g, q), column(A, g, q, True)
            out[:, m], bound[:, m], out[:, s], bound[:, s] = mean_and_stderr(terms[g, q], dterms[g, q])
    return BasketPathGreeksRef(out, bound, doubt_ind.sum(axis=1), doubt_arg.sum(axis=1), terms)


def draws(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int) -> tuple[np.ndarray, np.ndarray]:
    """(z, radius) [B, A, T, P] of the contracts' streams."""
    z, rad = br.drivers(br.stream_words(oracle, rows.shape[0], A, T, P, seed, ordinal0))
    return np.ascontiguousarray(z[:, :A, :, :P]), np.ascontiguousarray(rad[:, :A, :, :P])


def reference(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, *,
              weights: np.ndarray | None = None, corr: np.ndarray | None = None, math: str = "portable",
              normalize: bool = True, **wrong: bool) -> BasketPathGreeksRef:
    """smc_basket_greeks_paths for these contracts, and its bounds.  weights [A] or [B, A] (None: 1 / A), corr [A, A]
    or [B, A, A] (None: each row's rho)."""
    rows = np.asarray(rows, dtype=np.float64)
    z, rad = draws(oracle, rows, A, T, P, seed, ordinal0)
    return greeks(rows, A, T, z, rad, bp.weights_of(weights, rows.shape[0], A), gr.factors(rows, A, corr), math,
                  normalize=normalize, **wrong)


def prices(rows: np.ndarray, A: int, T: int, z: np.ndarray, radius: np.ndarray, w: np.ndarray, Lf: np.ndarray,
           normalize: bool) -> np.ndarray:
    """[B, 4]: basket_path_reference's own f64 prices of the four payoffs on the drivers z (for central differences on
    common drivers; the factor Lf stays fixed, the scales are recomputed from the bumped sample)."""
    x, rel = br.paths(rows, A, T, z, radius, br.PORTABLE, L=Lf)
    return bp.outputs(rows, A, x, rel, w, None, normalize).cols[:, [0, 1, 4, 5]]


def path_payoffs(rows: np.ndarray, A: int, T: int, z: np.ndarray, radius: np.ndarray, w: np.ndarray, Lf: np.ndarray,
                 normalize: bool) -> dict[str, np.ndarray]:
    """Per-path payoffs [4, B, P] (the PAYOFFS order) from basket_path_reference's scaled rows and levels, with the rows
    of the minimum and of the maximum [2, B, P]; their means are prices(...)'s columns."""
    rows = np.asarray(rows, dtype=np.float64)
    x, rel = br.paths(rows, A, T, z, radius, br.PORTABLE, L=Lf)
    xs, dxs, _, _ = bp.scaled_rows(rows, A, x, rel, normalize)
    b = bp.levels(xs, dxs, w)[0]
    K, Tm, r = fields(rows, A)[:3]
    df, Kc = np.exp(-r * Tm)[:, None], K[:, None]
    avg, mn, mx = b.mean(axis=1), b.min(axis=1), b.max(axis=1)
    pay = np.stack([df * np.maximum(Kc - avg, 0), df * np.maximum(avg - Kc, 0), df * np.maximum(Kc - mn, 0),
                    df * np.maximum(mx - Kc, 0)])
    return {"pay": pay, "rows_at": np.stack([b.argmin(axis=1), b.argmax(axis=1)]), "under": np.stack([avg, avg, mn, mx])}


def share_used(got: np.ndarray, ref: BasketPathGreeksRef, columns: list[int] | None = None) -> float:
    c = slice(None) if columns is None else columns
    return br.share_used(np.asarray(got)[:, c], ref.cols[:, c], ref.bound[:, c])
