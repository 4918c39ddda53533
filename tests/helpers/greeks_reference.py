"""An independent float64 reference of the single-asset pathwise Greeks (smc_gbm_greeks, greeks_kernel of csrc/gbm.hip),
with an a-priori bound on how far the f32 kernel may lie from it, in portable and in SMC_MATH_HW math.  numpy only.

What it shares with the kernel: the stream words, the normals and the paths (gbm_reference.stream_words, normals and
paths, so the terminal bound dxT comes with them) and the documented meaning of the 26 columns
(include/spectralmc_hip.h).  What it does not share: any arithmetic of the kernel or of its restatement
(tests/helpers/greeks_restate.py).  No log of a terminal value enters a Greek: the Brownian term comes from the drivers.

The model
---------
x = X0 exp(mu T + v W),  W = sqrt(dt) sum_t z_t,  dt = T / steps,  mu = r - d - v^2 / 2.  Hence, path by path,
    d ln x / d v = W - v T,   d ln x / d T = mu + v W / (2 T),   d ln x / d X0 = 1 / X0,   d ln x / d r = T.
RAW: xs = x.  NORMALIZE: xs = x F / mean_p(x) with F = X0 e^{(r - d) T}.  For v and T the derivative of ln xs is then
that of ln x less its x-weighted mean over the paths (the derivative of ln mean x), plus that of ln F: r - d for T, 0
for v.  The x-weighted mean is taken of the derivative itself (of W - v T, of mu + v W / (2 T)), not of a log return.
For X0 and r, x and F move alike, so d ln xs / d X0 = 1 / X0 and d ln xs / d r = T as under RAW.
With df = e^{-r T}, put = df max(K - xs, 0), call = df max(xs - K, 0), ip = 1{K > xs}, ic = 1{xs > K}, w = df xs:
    delta  -+ 1{.} w / X0                                    vega  -+ 1{.} w d ln xs / d v
    rho    -+ 1{.} T K df   (d/dr of df (K - xs): -T df (K - xs) - df xs T)
    theta  = -dV/dT:  r put + ip w d ln xs / d T,   r call - ic w d ln xs / d T
    gamma  = vega / (v T X0^2) (the lognormal identity), its standard error likewise.
Columns 0..9 are the means of these over the paths, 10..19 their standard errors sqrt(sample variance (n - 1) / P),
20 / 21 the prices, 22 / 23 their errors, 24 sum x, 25 sum x ln(x / X0) with ln(x / X0) = mu T + v W (0 under RAW).
Conventions of the header, applied as stated there: v == 0 gives vega = gamma = 0 and errors 0; T == 0 keeps mu / 2
(RAW) or r - d (NORMALIZE) as d ln xs / d T; v T == 0 gives gamma 0; P == 1 gives every error 0.

The bound
---------
Nothing is fitted to the kernel.  The inputs are the reference's own values, U = 2^-24, gbm_reference's MathEps
(PORTABLE or HW) for the paths, and the maxima of the two logs over q in [2^-8, 2^8) named in
tests/helpers/math_inputs.py (LogEps: relative outside [1 / sqrt 2, sqrt 2), absolute inside; PORTABLE_LOG the measured
maxima of log_pos, HW_LOG twice those of hw_log).  Two rules do all the propagation: a rounded product of a (within
da) and b (within db) lies within
    prod: |a| db + |b| da + da db + U (|a b| + the former)
of a b, and a rounded sum within
    add:  da + db + U (|a + b| + da + db).
* x within dxT (gbm_reference.paths).  X0 rounds to f32 (U relative) and q = fl(x / x0) rounds once more, so q carries
  the relative error eq = (1 + dxT / x) (1 + U) / (1 - U) - 1 and ln q moves by at most -log1p(-eq).  The log itself
  errs by LogEps at q; a q within eq of either end of [1 / sqrt 2, sqrt 2) is charged the larger of the two.  Together
  dL.  A q beyond [2^-8, 2^8) (the T v^2 corner of the hand-built rows, a wide Sobol draw) is charged the relative
  figure as well, by this reasoning and no sweep: both logs are a function of the mantissa, which the 16 swept
  exponents exhaust, plus the exponent times ln 2.  For log_pos, |e| >= 8 adds |e| |f32(ln 2) - ln 2| (2.8e-9 of
  |e| ln 2), the mantissa part keeps its absolute error (below 5e-8 + 2^-24 0.35) and fmaf rounds once (2^-24
  relative): under 8e-8 of |ln q| >= 7 ln 2, below LOG_POS_Q_MAX_REL.  For hw_log, v_log_f32 is documented to 1 ulp
  of log2 q (2^-23 relative away from q = 1) and the product with f32(ln 2) adds 2.8e-9 + 2^-24: 1.9e-7, below
  HW_LOG_Q_REL_BOUND.
* The constants 1 / X0, 1 / v, 1 / (2 T), r, mu / 2, av = -mu T / v - v T are f64 values rounded once (U relative).
  hv = fl(fl(L cv) + av) by prod and add: under RAW L cv and av cancel (their sum is W - v T), and the rules charge U
  against |L cv| and |av|, not against |hv|.  hT = fl(fl(L cT) + aT) likewise.
* NORMALIZE: Lbar = sumxl / sumx in f64.  sumxl adds f64(fl(x L)): each by prod from dxT and dL, the f64 sum P 2^-52
  sum |x L|; sumx within gbm_reference.row_sums' bound; so dLbar = (dsumxl + |Lbar| dsumx) / (sumx - dsumx).  av and
  aT are f64 functions of Lbar rounded once.
* df and F from gbm_reference.discount and forwards, xs from scaled (RAW: the kernel multiplies by 1, exactly).
  w = fl(df xs), wd = fl(w ix0), wv = fl(w hv), wt = fl(w hT) by prod; put and call by gbm_reference.payoff;
  crho = fl(df fl(T K)): the errors of df, T, K and two roundings; theta = fl(fl(rr payoff) +- wt) by prod and add.
* A path with |xs - K| <= dxs + |f32(K) - K| may have either indicator (the kernel's comparison K - xs > 0 is exact
  in its own values): each of its indicator terms carries its whole live value, plus that value's bound, as error.
  The count of such paths per contract is returned (doubt); a test may ask gbm_reference.count_ok of it.
* Means and standard errors by gbm_reference.mean_and_stderr.  gamma and its error: the vega bounds over v T X0^2,
  plus 4 2^-52 relative for the f64 division.
The float64 errors of the reference itself are orders below all of this and are left out.

The keyword arguments of `greeks` listed in WRONG are wrong readings, for the sensitivity test of
tests/test_greeks_reference.py only.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.helpers import gbm_reference as gref
from tests.helpers import math_inputs as mi
from tests.helpers.gbm_reference import U

COLS = 26
MEAN_COLS = list(range(10)) + [20, 21]
STDERR_COLS = list(range(10, 20)) + [22, 23]
SUM_COLS = [24, 25]
# the means apart: those that take no log (delta, rho, the prices) and those that do (vega, theta, gamma)
GROUPS = {"delta rho price": [0, 1, 4, 5, 20, 21], "vega theta gamma": [2, 3, 6, 7, 8, 9], "stderr": STDERR_COLS,
          "sums": SUM_COLS}
NAMES = ["put_delta", "call_delta", "put_vega", "call_vega", "put_rho", "call_rho", "put_theta", "call_theta",
         "put_gamma", "call_gamma"]
WRONG = ("no_vT", "aT_mu", "theta_off", "no_lbar", "plain_mean", "no_carry_theta", "no_r_payoff", "rho_carry", "rho_xs",
         "gamma_x0", "exchanged", "delta_k", "stderr_p", "dt_plus")
R2 = float(np.sqrt(0.5))


@dataclass(frozen=True)
class LogEps:
    rel: float   # |log - ln q| / |ln q| for q outside [1 / sqrt 2, sqrt 2)
    abs: float   # |log - ln q| inside it


PORTABLE_LOG = LogEps(mi.LOG_POS_Q_MAX_REL, mi.LOG_POS_Q_MAX_ABS)
HW_LOG = LogEps(mi.HW_LOG_Q_REL_BOUND, mi.HW_LOG_Q_ABS_BOUND)
LOGS = {"portable": PORTABLE_LOG, "hw": HW_LOG}


def prod(a, da, b, db):
    """Bound of a rounded f32 product of a (within da) and b (within db)."""
    e = np.abs(a) * db + np.abs(b) * da + da * db
    return e + U * (np.abs(a * b) + e)


def add(a, da, b, db):
    """Bound of a rounded f32 sum."""
    return da + db + U * (np.abs(a + b) + da + db)


def log_bound(q: np.ndarray, eq: np.ndarray, leps: LogEps) -> np.ndarray:
    """|log(q') - ln q| for any q' within the relative eq of q (q' a positive normal f32)."""
    assert np.all(q * (1.0 - eq) > 2.0 ** -126)
    lq = np.abs(np.log(q)) - np.log1p(-eq)          # the largest |ln q'|
    inside = (q * (1.0 - eq) >= R2) & (q * (1.0 + eq) < 1.0 / R2)
    outside = (q * (1.0 + eq) < R2) | (q * (1.0 - eq) >= 1.0 / R2)
    rel = leps.rel * lq
    return -np.log1p(-eq) + np.where(inside, leps.abs, np.where(outside, rel, np.maximum(rel, leps.abs)))


@dataclass
class GreeksRef:
    cols: np.ndarray    # [B, 26]
    bound: np.ndarray   # [B, 26]
    doubt: np.ndarray   # [B] paths whose indicator the bound leaves open
    slack64: np.ndarray  # [B, 26] what float64 arithmetic of the header's route may lose to cancellation (see tol64)
    xs: np.ndarray      # [B, P] scaled terminal values
    dxs: np.ndarray
    dxs_dtheta: dict    # name -> [B, P], d xs / d (X0, v, r, T): for the kink condition of a finite difference


def greeks(rows: np.ndarray, T: int, z: np.ndarray, radius: np.ndarray, eps: gref.MathEps = gref.PORTABLE,
           leps: LogEps = PORTABLE_LOG, *, normalize: bool = True, no_vT: bool = False, aT_mu: bool = False,
           theta_off: float = 0.0, no_lbar: bool = False, plain_mean: bool = False, no_carry_theta: bool = False,
           no_r_payoff: bool = False, rho_carry: bool = False, rho_xs: bool = False, gamma_x0: bool = False,
           exchanged: bool = False, delta_k: bool = False, stderr_p: bool = False, dt_plus: bool = False) -> GreeksRef:
    """The 26 columns for contract rows [B, 6] and their normals z, radius [B, T, P], with bounds."""
    rows = np.asarray(rows, dtype=np.float64)
    X0, K, Tm, r, d, v = gref.fields(rows)
    B, _, P = z.shape
    col = lambda a: np.asarray(a)[:, None]  # noqa: E731
    x, dx = gref.paths(rows, T, z, radius, eps)
    x, dx = np.ascontiguousarray(x[:, -1]), np.ascontiguousarray(dx[:, -1])
    W = col(np.sqrt(Tm / (T + 1 if dt_plus else T))) * z.sum(axis=1)
    mu = r - d - 0.5 * v * v
    L = col(mu * Tm) + col(v) * W                       # ln(x / X0), from the drivers
    live_v, live_T = col(v != 0.0), col(Tm != 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dv = np.where(live_v, W - (0.0 if no_vT else col(v * Tm)), 0.0)
        dT = np.where(live_T, col(mu) + col(v) * W / col(2.0 * Tm), col(mu / 2.0))
        ix0, cv, cT = 1.0 / X0, np.where(v != 0.0, 1.0 / v, 0.0), np.where(Tm != 0.0, 1.0 / (2.0 * Tm), 0.0)
    if aT_mu:
        dT = dT + col(mu / 2.0)
    dT = dT + theta_off
    sumx, dsumx = gref.row_sums(x, dx)
    sumxl, dsumxl = np.zeros(B), np.zeros(B)
    df, edf = gref.discount(rows)
    F, eF = gref.forwards(rows, T)
    F, eF = F[:, -1], eF[:, -1]
    # the log the kernel takes, and the constants of hv and hT
    eq = (1.0 + dx / x) * (1.0 + U) / (1.0 - U) - 1.0
    dL = log_bound(x / col(X0), eq, leps)
    if normalize:
        xL = x * L
        sumxl = xL.sum(axis=1)
        dsumxl = prod(x, dx, L, dL).sum(axis=1) + P * 2.0 ** -52 * np.abs(xL).sum(axis=1)
        lbar = sumxl / sumx
        dlbar = (dsumxl + np.abs(lbar) * dsumx) / (sumx - dsumx)
        wmean = (lambda a: col(a.mean(axis=1))) if plain_mean else (lambda a: col((x * a).sum(axis=1) / sumx))
        if not no_lbar:
            dv = np.where(live_v, dv - wmean(dv), 0.0)
            dT = dT - wmean(dT)
        dT = dT + (0.0 if no_carry_theta else col(r - d))
        dT = np.where(live_T, dT, col(r - d) + theta_off)
        av = -lbar * cv
        dav = dlbar * cv * (1.0 + U) + U * np.abs(av)
        aT = np.where(Tm != 0.0, -lbar * cT + (r - d), r - d)
        daT = dlbar * cT * (1.0 + U) + U * np.abs(aT)
        xs, dxs = gref.scaled(x, dx, sumx, dsumx, F, eF)
    else:
        av = np.where(v != 0.0, -mu * Tm * cv - v * Tm, 0.0)
        aT = mu / 2.0
        dav, daT = U * np.abs(av), U * np.abs(aT)
        xs, dxs = x, dx
    Lcv, Lct = L * col(cv), L * col(cT)
    dhv = add(Lcv, prod(L, dL, col(cv), col(U * cv)), col(av), col(dav))
    dhT = add(Lct, prod(L, dL, col(cT), col(U * cT)), col(aT), col(daT))
    # per-path values
    put, dput = gref.payoff(1.0, col(K), xs, dxs, col(df), col(edf))
    call, dcall = gref.payoff(-1.0, col(K), xs, dxs, col(df), col(edf))
    w = col(df) * xs
    dw = prod(col(df), col(df * edf), xs, dxs)
    one = (1.0 / K) if delta_k else ix0
    wd, dwd = w * col(one), prod(w, dw, col(ix0), col(U * ix0))
    wv, dwv = w * dv, prod(w, dw, dv, dhv)
    wt, dwt = w * dT, prod(w, dw, dT, dhT)
    dfr, edfr = gref.discount(rows, carry=True) if rho_carry else (df, edf)
    crho = np.broadcast_to(col(Tm * K * dfr), xs.shape)
    dcrho = np.broadcast_to(col(Tm * K * dfr * gref.compose(edfr, U, gref.f32_error(K) / K, U, U)), xs.shape)
    if rho_xs:
        crho = col(Tm * dfr) * xs
    ip, ic = col(K) - xs > 0.0, xs - col(K) > 0.0
    open_ = np.abs(xs - col(K)) <= dxs + col(gref.f32_error(K))
    if exchanged:
        ip, ic = ic, ip
    rr, drr = col(0.0 * r if no_r_payoff else r), col(gref.f32_error(r))
    rp, drp = rr * put, prod(rr, drr, put, dput)
    rc, drc = rr * call, prod(rr, drr, call, dcall)

    def gated(ind, s, ds, sign):
        """(sign s where ind else 0, its bound): a path in doubt carries the whole live value as error."""
        return np.where(ind, sign * s, 0.0), np.where(open_, np.abs(s) + ds, np.where(ind, ds, 0.0))

    tp, dtp = gated(ip, wt, dwt, 1.0)
    tc, dtc = gated(ic, wt, dwt, -1.0)
    terms = [gated(ip, wd, dwd, -1.0), gated(ic, wd, dwd, 1.0), gated(ip, wv, dwv, -1.0), gated(ic, wv, dwv, 1.0),
             gated(ip, crho, dcrho, -1.0), gated(ic, crho, dcrho, 1.0),
             (rp + tp, add(rp, drp, tp, dtp)), (rc + tc, add(rc, drc, tc, dtc)), (put, dput), (call, dcall)]
    cols, bound, slack64 = np.zeros((B, COLS)), np.zeros((B, COLS)), np.zeros((B, COLS))
    for i, (t, dt_) in enumerate(terms):
        m, dm, se, dse = gref.mean_and_stderr(t, dt_)
        if stderr_p and P > 1:
            se = se * np.sqrt((P - 1.0) / P)
        a, b = (i, 10 + i) if i < 8 else (12 + i, 14 + i)
        cols[:, a], bound[:, a], cols[:, b], bound[:, b] = m, dm, se, dse
        if P > 1:  # D = sum t^2 - P m^2 in f64 is off by at most H, and sqrt(D + H) - sqrt(D) <= min(sqrt H, H / (2 sqrt D))
            H = 4 * P * 2.0 ** -53 * np.square(t).sum(axis=1)
            D = np.square(t - col(m)).sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                slack64[:, b] = np.minimum(np.sqrt(H), np.where(D > 0.0, H / (2.0 * np.sqrt(D)), np.inf)) / np.sqrt(P * (P - 1.0))
    # L cv + av and L cT + aT cancel in any arithmetic: 2^-53 of each operand and of the sum, twice over for Lbar's share
    slack64[:, 2] = slack64[:, 3] = 8 * 2.0 ** -53 * (np.abs(w) * (np.abs(Lcv) + np.abs(col(av)))).mean(axis=1)
    slack64[:, 6] = slack64[:, 7] = 8 * 2.0 ** -53 * (np.abs(w) * (np.abs(Lct) + np.abs(col(aT)))).mean(axis=1)
    vt = v * Tm
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(vt == 0.0, np.inf, vt * X0 * (1.0 if gamma_x0 else X0))
    for a in (2, 3, 12, 13):
        cols[:, a + 6] = cols[:, a] / den
        bound[:, a + 6] = bound[:, a] / den + 4 * 2.0 ** -52 * np.abs(cols[:, a + 6])
        slack64[:, a + 6] = slack64[:, a] / den
    cols[:, 24], bound[:, 24] = sumx, dsumx
    cols[:, 25], bound[:, 25] = sumxl, dsumxl
    dxs_dtheta = {"X0": xs * col(ix0), "v": xs * dv, "r": xs * col(Tm), "T": xs * dT}
    return GreeksRef(cols, bound, open_.sum(axis=1), slack64, xs, dxs, dxs_dtheta)


def concat(parts: list[GreeksRef]) -> GreeksRef:
    cat = lambda name: np.concatenate([getattr(p, name) for p in parts])  # noqa: E731
    return GreeksRef(cat("cols"), cat("bound"), cat("doubt"), cat("slack64"), cat("xs"), cat("dxs"),
                     {k: np.concatenate([p.dxs_dtheta[k] for p in parts]) for k in parts[0].dxs_dtheta})


def reference(oracle, rows: np.ndarray, T: int, P: int, seed: int, ordinal0: int, *, math: str = "portable",
              normalize: bool = True, f64: bool = False, **wrong) -> GreeksRef:
    """smc_gbm_greeks for these contracts in float64, and its bounds in the given math ("portable" or "hw").
    f64: on the uniforms of the float64 engine (gbm_reference.normals); the bounds then mean nothing, the float64
    kernels are held at the project's float64 tolerance."""
    rows = np.asarray(rows, dtype=np.float64)
    eps = {"portable": gref.PORTABLE, "hw": gref.HW}[math]
    block = max(1, gref.ELEMENTS // (T * P))
    parts = []
    for b0 in range(0, rows.shape[0], block):
        blk = rows[b0:b0 + block]
        z, rad = gref.normals(gref.stream_words(oracle, blk.shape[0], T, P, seed, ordinal0 + b0), T, P, f64=f64)
        parts.append(greeks(blk, T, z, rad, eps, LOGS[math], normalize=normalize, **wrong))
    return concat(parts)


def prices(rows: np.ndarray, T: int, z: np.ndarray, normalize: bool) -> np.ndarray:
    """[B, 2] the Monte-Carlo put and call of gbm_reference on the normals z [B, T, P]: the function the Greeks
    differentiate, for central differences on fixed stream words."""
    x, dx = gref.paths(rows, T, z, np.abs(z), gref.PORTABLE)
    ref = gref.outputs(rows, x, dx, normalize=normalize)
    return ref.price[:, :2]


def tol64(ref: GreeksRef, rtol: float, atol: float) -> np.ndarray:
    """[B, 26] the tolerance of a float64 evaluation: atol + rtol |want|, plus slack64 where float64 arithmetic of
    the header's route itself cancels (a standard error whose terms are all alike, D = sum t^2 - P m^2; the vega and
    theta weights L cv + av, L cT + aT, which vanish altogether at P = 1 under NORMALIZE).  slack64 is built from the
    reference's values and 2^-53 alone."""
    return atol + rtol * np.abs(ref.cols) + ref.slack64


def shares(got: np.ndarray, ref: GreeksRef) -> dict[str, float]:
    """The largest share of the bound used per column group."""
    return {k: gref.share_used(got[:, c], ref.cols[:, c], ref.bound[:, c]) for k, c in GROUPS.items()}
