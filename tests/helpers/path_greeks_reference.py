"""An independent float64 reference of the pathwise Greeks of the Asian and lookback options (smc_gbm_greeks_paths,
path_greeks_kernel of csrc/gbm.hip), with an a-priori bound on how far the kernel may lie from it: the f32 kernel in
portable and in SMC_MATH_HW math, and, evaluated in long double, the f64 kernel.  numpy only.

What it shares with the kernel: the stream words, the normals and the paths (gbm_reference.stream_words, normals and
paths, so the row bounds dx come with them), gbm_reference's row sums, forwards, scales, payoff and mean_and_stderr,
and the documented meaning of the 40 columns (include/spectralmc_hip.h).  What it does not share: any arithmetic of
the kernel or of its restatement (tests/helpers/path_greeks_restate.py).  No log of a simulated value enters a
derivative: the Brownian terms come from the drivers.

The model
---------
Row t (0-based) of steps rows: tau_t = (t + 1) T / steps, fr_t = (t + 1) / steps, W_t = sqrt(dt) sum_{s <= t} z_s,
x_t = X0 exp(mu tau_t + v W_t), mu = r - d - v^2 / 2.  Path by path and row by row
    d ln x_t / d v = W_t - v tau_t       d ln x_t / d T = mu fr_t + v W_t / (2 T)   (every date moves with T)
    d ln x_t / d X0 = 1 / X0             d ln x_t / d r = tau_t.
RAW: xs_t = x_t.  NORMALIZE: xs_t = x_t F_t / mean_p(x_t), F_t = X0 e^{(r - d) tau_t}: for v and T the derivative of
ln xs_t is that of ln x_t less its x_t-weighted mean over the paths (the derivative of ln mean x_t), plus that of
ln F_t: (r - d) fr_t for T, 0 for v.  For X0 and r, x_t, F_t and the mean move alike.
Underlyings: the Asian average u = mean_t xs_t with d u = mean_t (xs_t d ln xs_t); the lookback call's u = max_t xs_t
and the put's min_t xs_t, with d u = xs_t* d ln xs_t* at the row t* of the extreme (the first one on a tie).
With df = e^{-r T}, put = df max(K - u, 0), call = df max(u - K, 0), ip = 1{K > u}, ic = 1{u > K}:
    delta  -+ 1{.} df u / X0                         vega  -+ 1{.} df du/dv
    rho    -T put - ip df du/dr,  -T call + ic df du/dr
    theta  = -dV/dT:  r put + ip df du/dT,  r call - ic df du/dT.
Columns 0..15 are the means over the paths (delta, vega, rho, theta; Asian put, Asian call, lookback put, lookback
call inside each), 16..31 their standard errors, 32..35 the prices, 36..39 theirs.  Conventions of the header:
v == 0 gives d ln xs_t / d v = 0; T == 0 keeps mu fr_t / 2 (RAW) or (r - d) fr_t (NORMALIZE) as d ln xs_t / d T.

The bound
---------
Nothing is fitted to the kernel.  The inputs are the reference's own values, the unit roundoff u of the format,
gbm_reference's typings for the paths and greeks_reference's LogEps for the log (the library log of the f64 kernel is
charged 2 ulp: 4 u relative, 4 u 0.35 absolute inside [1 / sqrt 2, sqrt 2)).  greeks_reference's two rules, prod and
add, with u as a parameter, do the propagation.
* x_t within dx_t (gbm_reference.paths), q = fl(x_t / fl(X0)), dL from greeks_reference.log_bound, row by row.
* The row constants: tr_t = tau_t rounded once (the f64 grid point dt + t (T - dt) / (steps - 1) carries 5 roundings
  of its own: 6 u in f64), av_t and aT_t f64 values rounded once; under NORMALIZE Lbar_t = sumxl_t / sumx_t with
  greeks_reference's dLbar, per row.  hv = fl(fl(L cv) + av), hT = fl(fl(L cT) + aT) by prod and add.
* xs_t from gbm_reference.scaled; the products xs hv, xs hT, xs tr by prod; a running sum of n terms in the format
  and the division by steps: n roundings against the sum of the absolute terms.
* df u, (df u) / X0, df gv, df gT, df gr by prod; put and call by gbm_reference.payoff; Tr put and rr put by prod,
  the sums by add.
* A path with |u - K| <= du + |fl(K) - K| may have either indicator: each indicator term of it carries its whole live
  value, plus that value's bound, as error (doubt_ind counts such paths, per payoff family).
* The lookback row: every row whose value lies within the two rows' bounds of the extreme is a candidate; the kernel
  takes one of them, so the path is charged the largest distance of a candidate's term (plus its bound) from the
  reference's.  doubt_arg counts the paths with more than one candidate.
* A flat contract (v == 0 with r == d, or T == 0) keeps every row on fl(X0) exactly in the kernel too (the exponent
  is exactly 0, 2^0 = 1, the scale F_t / mean is 1): its rows tie exactly, the first row wins in the kernel as here,
  and nothing is in doubt.
* Means and standard errors by gbm_reference.mean_and_stderr.

The keyword arguments of `greeks` listed in WRONG are wrong readings, for the sensitivity test of
tests/test_path_greeks_reference.py only.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.helpers import gbm_reference as gref
from tests.helpers import greeks_reference as gk

COLS = 40
PAYOFFS = ("asian_put", "asian_call", "lookback_put", "lookback_call")
GREEKS = ("delta", "vega", "rho", "theta", "price")
MEAN_COLS = list(range(16)) + [32, 33, 34, 35]
STDERR_COLS = list(range(16, 32)) + [36, 37, 38, 39]
WRONG = ("no_lbar", "plain_mean", "terminal_tau", "last_tie", "maturity_only", "rho_no_discount", "with_x0",
         "exchanged")
F64_LOG = gk.LogEps(4 * gref.U64, 4 * gref.U64 * 0.35)
TYPINGS = {"portable": (gref.F32_PORTABLE, gk.PORTABLE_LOG), "hw": (gref.F32_HW, gk.HW_LOG),
           "f64": (gref.F64_ENGINE, F64_LOG)}


def column(greek: int, payoff: int, stderr: bool = False) -> int:
    if greek == 4:
        return (36 if stderr else 32) + payoff
    return (16 if stderr else 0) + 4 * greek + payoff


def prod(a, da, b, db, u):
    e = np.abs(a) * db + np.abs(b) * da + da * db
    return e + u * (np.abs(a * b) + e)


def add(a, da, b, db, u):
    return da + db + u * (np.abs(a + b) + da + db)


@dataclass
class PathGreeksRef:
    cols: np.ndarray       # [B, 40]
    bound: np.ndarray      # [B, 40]
    doubt_ind: np.ndarray  # [B] paths with an indicator the bound leaves open (Asian or lookback)
    doubt_arg: np.ndarray  # [B] paths whose row of the maximum or of the minimum the bound leaves open
    terms: np.ndarray      # [5, 4, B, P] per-path terms (greek, payoff)
    rows_at: np.ndarray    # [2, B, P] the rows of the minimum and of the maximum
    under: np.ndarray      # [3, B, P] the underlyings: average, minimum, maximum


def _row_state(rows, T, z, radius, ty, leps, normalize, w):
    """Rows xs, their bounds, the three log-derivatives per row with the bounds of the kernel's versions."""
    fmt = ty.fmt
    u, real = fmt.u, z.dtype.type
    X0, K, Tm, r, d, v = (f.astype(z.dtype) for f in gref.fields(rows))
    B, _, P = z.shape
    c2 = lambda a: np.asarray(a)[:, None]            # noqa: E731  [B] -> [B, 1]
    c3 = lambda a: np.asarray(a)[:, None, None]      # noqa: E731  [B] -> [B, 1, 1]
    x, dx = gref.paths(rows, T, z, radius, ty)
    flat = ((v == 0) & (r == d)) | (Tm == 0)
    dx = np.where(c3(flat), c3(fmt.input_error(X0)), dx)
    fr = (np.arange(1, T + 1).astype(z.dtype) / real(T))[None, :]                  # [1, T]
    tau = c2(Tm) * fr                                                               # [B, T]
    if w["terminal_tau"]:
        tau, fr = np.broadcast_to(c2(Tm), tau.shape), np.ones_like(fr)
    W = np.cumsum(c3(np.sqrt(Tm / T)) * z, axis=1)
    mu = r - d - v * v / 2
    L = (c2(mu) * (c2(Tm) * (np.arange(1, T + 1).astype(z.dtype) / real(T))[None, :]))[:, :, None] + c3(v) * W
    live_v, live_T = c3(v != 0), c3(Tm != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        hv = np.where(live_v, W - (c2(v) * tau)[:, :, None], 0)
        hT = np.where(live_T, (c2(mu) * fr)[:, :, None] + c3(v) * W / c3(2 * Tm), (c2(mu / 2) * fr)[:, :, None])
        if w["maturity_only"]:
            hT = hT * (np.arange(T) == T - 1)[None, :, None]
        ix0 = 1 / X0
        cv = np.where(v != 0, 1 / v, 0)
        cT = np.where(Tm != 0, 1 / (2 * Tm), 0)
    # the log the kernel takes
    eq = (1 + dx / x) * (1 + u) / (1 - u) - 1
    dL = gk.log_bound(x / c3(X0), eq, leps)
    dL = np.where(c3(flat), 0, dL)                   # q = 1 exactly: both logs give exactly 0
    sumx, dsumx = gref.row_sums(x, dx, fmt=fmt)      # [B, T]
    F, eF = gref.forwards(rows, T, fmt=fmt)
    if normalize:
        xL = x * L
        sumxl = xL.sum(axis=2)
        dsumxl = prod(x, dx, L, dL, u).sum(axis=2) + P * 2.0 ** -52 * np.abs(xL).sum(axis=2)
        lbar = sumxl / sumx
        dlbar = (dsumxl + np.abs(lbar) * dsumx) / (sumx - dsumx)
        if w["plain_mean"]:
            wmean = lambda a: a.mean(axis=2, keepdims=True)                       # noqa: E731
        else:
            wmean = lambda a: ((x * a).sum(axis=2) / sumx)[:, :, None]            # noqa: E731
        if not w["no_lbar"]:
            hv = np.where(live_v, hv - wmean(hv), 0)
            hT = hT - wmean(hT)
        carry = (c2(r - d) * fr)[:, :, None]
        if w["maturity_only"]:
            carry = carry * (np.arange(T) == T - 1)[None, :, None]
        hT = np.where(live_T, hT + carry, carry)
        av = -lbar * c2(cv)
        dav = dlbar * c2(cv) * (1 + u) + u * np.abs(av)
        aT = np.where(c2(Tm) != 0, -lbar * c2(cT), 0) + c2(r - d) * fr
        daT = dlbar * c2(cT) * (1 + u) + u * np.abs(aT)
        xs, dxs = gref.scaled(x, dx, sumx, dsumx, F, eF, fmt=fmt)
        xs = np.where(c3(flat), x, xs)
        dxs = np.where(c3(flat), dx, dxs)
    else:
        av = np.where(c2(v) != 0, -c2(mu) * tau * c2(cv) - c2(v) * tau, 0)
        aT = c2(mu / 2) * fr
        dav, daT = u * np.abs(av), u * np.abs(aT)
        xs, dxs = x, dx
    Lcv, LcT = L * c3(cv), L * c3(cT)
    dhv = add(Lcv, prod(L, dL, c3(cv), c3(u * cv), u), av[:, :, None], dav[:, :, None], u)
    dhT = add(LcT, prod(L, dL, c3(cT), c3(u * cT), u), aT[:, :, None], daT[:, :, None], u)
    dhv = np.where(live_v, dhv, 0)                   # cv = av = 0 exactly: hv = fl(L 0 + 0) = 0
    hr = np.broadcast_to(tau[:, :, None], xs.shape)
    dhr = np.broadcast_to(((1 if fmt.inputs_round else 6) * u * np.abs(tau))[:, :, None], xs.shape)
    return dict(xs=xs, dxs=dxs, hv=hv, dhv=dhv, hT=hT, dhT=dhT, hr=hr, dhr=dhr, flat=flat, ix0=ix0, fmt=fmt)


def _payoff_terms(rows, fmt, sign, un, dun, g, dg, w):
    """The five per-path terms of one payoff and their bounds from the underlying (un, dun) and its three
    derivatives g = (gv, gT, gr) with bounds dg; the arrays may carry any leading shape [B, ...]."""
    u = fmt.u
    X0, K, Tm, r, d, v = (f.astype(un.dtype) for f in gref.fields(rows))
    df, edf = gref.discount(rows, fmt=fmt)
    ex = lambda a: np.asarray(a).reshape((-1,) + (1,) * (un.ndim - 1))            # noqa: E731
    pay, dpay = gref.payoff(sign, ex(K), un, dun, ex(df), ex(edf), fmt=fmt)
    ind = sign * (ex(K) - un) > 0
    open_ = np.abs(un - ex(K)) <= dun + ex(fmt.input_error(K))
    ddf = ex(df * edf)
    wgt, dwgt = ex(df) * un, prod(ex(df), ddf, un, dun, u)
    ix0 = ex(1 / X0)
    live = [(wgt * ix0, prod(wgt, dwgt, ix0, u * ix0, u))]
    live += [(ex(df) * gi, prod(ex(df), ddf, gi, dgi, u)) for gi, dgi in zip(g, dg)]

    def gated(s, ds, sg):
        return np.where(ind, sg * s, 0), np.where(open_, np.abs(s) + ds, np.where(ind, ds, 0))

    (wd, dwd), (wv, dwv), (wT, dwT), (wr, dwr) = live
    delta, vega = gated(wd, dwd, -sign), gated(wv, dwv, -sign)
    gr_, gT_ = gated(wr, dwr, -sign), gated(wT, dwT, sign)
    Tp = -ex(Tm) * pay
    dTp = prod(ex(Tm), ex(fmt.input_error(Tm)), pay, dpay, u)
    if w["rho_no_discount"]:
        Tp = 0 * Tp
    rho = (Tp + gr_[0], add(Tp, dTp, gr_[0], gr_[1], u))
    rp, drp = ex(r) * pay, prod(ex(r), ex(fmt.input_error(r)), pay, dpay, u)
    theta = (rp + gT_[0], add(rp, drp, gT_[0], gT_[1], u))
    return [delta, vega, rho, theta, (pay, dpay)], open_


def greeks(rows: np.ndarray, T: int, z: np.ndarray, radius: np.ndarray, math: str = "portable", *,
           normalize: bool = True, **wrong: bool) -> PathGreeksRef:
    """The 40 columns for contract rows [B, 6] and their normals z, radius [B, T, P], with bounds."""
    assert set(wrong) <= set(WRONG)
    w = {k: bool(wrong.get(k, False)) for k in WRONG}
    ty, leps = TYPINGS[math]
    rows = np.asarray(rows, dtype=np.float64)
    st = _row_state(rows, T, z, radius, ty, leps, normalize, w)
    fmt, u = st["fmt"], st["fmt"].u
    xs, dxs = st["xs"], st["dxs"]
    B, _, P = xs.shape
    hs = [(st["hv"], st["dhv"]), (st["hT"], st["dhT"]), (st["hr"], st["dhr"])]
    if w["with_x0"]:  # X0 as row 0: it moves with X0 alone
        X0 = gref.fields(rows)[0].astype(xs.dtype)
        first = np.broadcast_to(X0[:, None, None], (B, 1, P))
        zero = np.zeros((B, 1, P), dtype=xs.dtype)
        xs, dxs = np.concatenate([first, xs], axis=1), np.concatenate([zero, dxs], axis=1)
        hs = [(np.concatenate([zero, h], axis=1), np.concatenate([zero, dh], axis=1)) for h, dh in hs]
    n = xs.shape[1]
    per_row = [(xs * h, prod(xs, dxs, h, dh, u)) for h, dh in hs]                 # xs d ln xs, [B, n, P]

    def averaged(val, dval):
        S, dS, A = val.sum(axis=1), dval.sum(axis=1), np.abs(val).sum(axis=1)
        return S / n, (dS + ((1 + u) ** n - 1) * (A + dS)) / n

    ua, dua = averaged(xs, dxs)
    ga = [averaged(v_, dv_) for v_, dv_ in per_row]
    terms = np.zeros((5, 4, B, P), dtype=xs.dtype)
    dterms = np.zeros_like(terms)
    doubt_ind = np.zeros((B, P), dtype=bool)
    for q, sign in ((0, 1.0), (1, -1.0)):
        t5, open_ = _payoff_terms(rows, fmt, sign, ua, dua, [g for g, _ in ga], [dg for _, dg in ga], w)
        doubt_ind |= open_
        for g, (val, dval) in enumerate(t5):
            terms[g, q], dterms[g, q] = val, dval
    # the lookback payoffs: the terms at every row, then the row of the extreme and its candidates
    flat = st["flat"][:, None, None]
    doubt_arg = np.zeros((B, P), dtype=bool)
    rows_at = np.zeros((2, B, P), dtype=np.int64)
    under = np.zeros((3, B, P), dtype=xs.dtype)
    under[0] = ua
    for q, sign, take_max in ((2, 1.0, False), (3, -1.0, True)):
        if w["exchanged"]:
            take_max = not take_max
        key = xs if take_max else -xs
        if w["last_tie"]:
            at = n - 1 - np.argmax(key[:, ::-1], axis=1)
        else:
            at = np.argmax(key, axis=1)                                            # the first row of the extreme
        best = np.take_along_axis(key, at[:, None, :], axis=1)
        dbest = np.take_along_axis(dxs, at[:, None, :], axis=1)
        cand = np.where(flat, np.arange(n)[None, :, None] == at[:, None, :], best - key <= dxs + dbest)
        doubt_arg |= cand.sum(axis=1) > 1
        t5, open_ = _payoff_terms(rows, fmt, sign, xs, dxs, [g for g, _ in per_row], [dg for _, dg in per_row], w)
        doubt_ind |= np.take_along_axis(open_, at[:, None, :], axis=1)[:, 0]
        for g, (val, dval) in enumerate(t5):
            ref = np.take_along_axis(val, at[:, None, :], axis=1)
            spread = np.where(cand, np.abs(val - ref) + dval, 0).max(axis=1)
            terms[g, q], dterms[g, q] = ref[:, 0], spread
        rows_at[1 if take_max else 0] = at
        under[2 if take_max else 1] = np.take_along_axis(xs, at[:, None, :], axis=1)[:, 0]
    cols, bound = np.zeros((B, COLS), dtype=xs.dtype), np.zeros((B, COLS), dtype=xs.dtype)
    for g in range(5):
        for q in range(4):
            a, b = column(g, q), column(g, q, True)
            cols[:, a], bound[:, a], cols[:, b], bound[:, b] = gref.mean_and_stderr(terms[g, q], dterms[g, q])
    return PathGreeksRef(cols, bound, doubt_ind.sum(axis=1), doubt_arg.sum(axis=1), terms, rows_at, under)


def arg_ok(doubt_arg: np.ndarray, P: int) -> bool:
    """The condition on the inputs a test may use: at most max(2, P / 128) paths of each contract whose row of an
    extreme the bound leaves open."""
    return bool(np.all(doubt_arg <= max(2, P // 128)))


def draws(oracle, rows: np.ndarray, T: int, P: int, seed: int, ordinal0: int, math: str = "portable"):
    ty = TYPINGS[math][0]
    assert gref.LONGDOUBLE_OK or not ty.f64_normals
    return gref.normals(gref.stream_words(oracle, rows.shape[0], T, P, seed, ordinal0), T, P, f64=ty.f64_normals,
                        longdouble=ty.f64_normals)


def reference(oracle, rows: np.ndarray, T: int, P: int, seed: int, ordinal0: int, *, math: str = "portable",
              normalize: bool = True, **wrong: bool) -> PathGreeksRef:
    """smc_gbm_greeks_paths for these contracts, and its bounds, in the given math ("portable", "hw" or "f64": the
    f64 kernel, evaluated in long double)."""
    rows = np.asarray(rows, dtype=np.float64)
    z, rad = draws(oracle, rows, T, P, seed, ordinal0, math)
    return greeks(rows, T, z, rad, math, normalize=normalize, **wrong)


# ---- the function the Greeks differentiate, for central differences on fixed normals ----------------------------------
def payoffs(rows: np.ndarray, T: int, z: np.ndarray, normalize: bool) -> dict[str, np.ndarray]:
    """Per-path payoffs [4, B, P] (the PAYOFFS order) of contract rows on the normals z [B, T, P], in float64, the
    scales recomputed from this sample; with the rows of the minimum and maximum and the underlyings."""
    X0, K, Tm, r, d, v = gref.fields(rows)
    c3 = lambda a: a[:, None, None]  # noqa: E731
    tau = Tm[:, None] * np.arange(1, T + 1)[None, :] / T
    x = c3(X0) * np.exp(((r - d - v * v / 2)[:, None] * tau)[:, :, None] + c3(v * np.sqrt(Tm / T)) * np.cumsum(z, axis=1))
    if normalize:
        x = x * (X0[:, None] * np.exp((r - d)[:, None] * tau) / x.mean(axis=2))[:, :, None]
    df = np.exp(-r * Tm)[:, None]
    avg, mn, mx = x.mean(axis=1), x.min(axis=1), x.max(axis=1)
    Kc = K[:, None]
    pay = np.stack([df * np.maximum(Kc - avg, 0), df * np.maximum(avg - Kc, 0), df * np.maximum(Kc - mn, 0),
                    df * np.maximum(mx - Kc, 0)])
    return {"pay": pay, "rows_at": np.stack([x.argmin(axis=1), x.argmax(axis=1)]), "under": np.stack([avg, mn, mx])}
