"""An independent float64 reference of the correlated multi-asset (basket) engine, with an a-priori bound on how
far the f32 kernels of csrc/basket.hip may lie from it.  numpy only.

What it shares with the kernels: the integer words of the path streams (oracle.stream_u32 / stream_u32_groups:
Philox pinned by the Random123 KAT, MWC64X by its Python restatement in tests/test_oracle.py) and the documented
meaning of the engine (csrc/smc_rng.h, DESIGN.md section 8, include/spectralmc_hip.h).  What it does not share: any
arithmetic.  No folded b_i L_ik coefficients, no log2 units, no per-step exp2, no Banachiewicz loop, and no call of
oracle.basket_cholesky, oracle.basket_kernel or oracle.basket_reference_targets.

The model
---------
Contract row [3A + 4]: K, T, r, rho, X0[A], d[A], v[A].  Path p of contract b belongs to group p // 4 of the stream
(seed, ordinal0 + b, group); a group's words are consumed in the order step, path within the group, pair, two words
(a, b) per pair and ceil(A / 2) pairs per path and step.  A pair gives two standard normals by Box-Muller on
u1 = 1 - (a >> 9) 2^-23 in (0, 1] and the angle (b >> 9) 2^-23 revolutions: radius sqrt(-2 ln u1), the cosine to
driver 2 pair, the sine to driver 2 pair + 1 (an odd A has no use for its last sine).  With C = (1 - rho) I + rho 11^T
= L L^T (numpy.linalg.cholesky; at the documented singular corner A = 2, rho = 1 that routine fails and the factor
[[1, 0], [1, 0]] is written out) and dt = T / steps,
    x_i(t) = X0_i exp( sum_{s <= t} [ (r - d_i - v_i^2 / 2) dt + v_i sqrt(dt) (L z(s))_i ] ).
Terminal sums tot_i = sum_p x_i(T, p).  Under NORMALIZE the scaled terminal values are xs_i = x_i F_i / (tot_i / P)
with the forward F_i = X0_i e^{(r - d_i) T}, under RAW xs_i = x_i.  Per path bk = (1 / A) sum_i xs_i, mx = max_i xs_i,
mn = min_i xs_i, and the payoffs df max(K - u, 0), df max(u - K, 0) with df = e^{-r T} for u = bk, mx, mn.  The 18
columns of smc_basket_price are their means, the standard errors sqrt(sample variance / P) (0 at P = 1), the means of
bk, mx, mn, the share of paths with bk < K and the intrinsic values of the basket put and call at
Fb = (1 / A) sum_i F_i.  The training target is numpy.fft.fft of the mean over the M rows of the basket put laid out
as [M, N] (path p: row p // N, column p % N).

The bound
---------
Nothing below is fitted to a kernel or to the oracle's kernel mode: the inputs are the reference's own intermediate
values, the f32 unit roundoff U = 2^-24, and the maximum errors of the device math functions that the sweeps of
tests/test_math_accuracy.py (portable) and tests/test_gpu_math.py (SMC_MATH_HW: twice the measured maxima) assert,
by the names of tests/helpers/math_inputs.py: eps_radius, eps_sincos (absolute) and eps_exp2 (relative).

One step of one asset in the kernel: y = a + sum_{k <= i} c_k z_k in log2 units (a = drift dt log2 e, c_k =
v sqrt(dt) log2 e L_ik, each rounded once to f32: relative U each), an fma chain of at most A roundings of partial
sums that are each at most |a| + sum |c_k z_k| in magnitude, so with exact drivers y is off by at most
(A + 2) U (|a| + sum_k |c_k z_k|).  A driver z = radius * trig is off by at most
    eps_z = eps_radius + radius eps_sincos + U |z|
(the radius error against a trig value of at most 1, the trig error against the radius, the product's rounding); under
SMC_MATH_HW the kernel's radius is sqrt(-log2 u1), the constant sqrt(2 ln 2) sits in c_k, and eps_radius is measured
on their product, so the same expression holds.  Hence
    eps_y = (A + 2) U (|a| + sum_k |c_k z_k|) + sum_k |c_k| eps_z,k.
x *= 2^y then multiplies the relative error by e^{ln 2 eps_y} (1 + eps_exp2) (1 + U): the exponent's error, the exp2
kernel, the product's rounding.  An element of a stored path after t steps therefore lies within the relative bound
    expm1( sum_{s <= t} [ ln 2 eps_y(s) + log1p(eps_exp2) + log1p(U) ] + log1p(U) ),
the last term being the rounding of X0 to f32: to first order the sum over the steps of ln 2 eps_y + eps_exp2 + U,
plus U.  The float64 errors of the reference itself (1e-15 per operation) are five orders below and are left out.

Everything after the terminal values is propagation.  delta_x = x rel.
* Terminal sum: the kernel adds a lane's 4 paths in f32 (3 roundings of a partial sum of positive terms) and the rest
  in f64: sum delta_x + 3 U sum (x + delta_x) + P 2^-52 sum x.
* Forward and discount: exp_any(f32(g) f32(T)) = exp2_any of a product of five rounded factors (g, T, their product,
  the f32 constant log2 e, the second product), so e^{g T} carries expm1(5 U' |g T|) with U' = log1p(U), eps_exp2 of
  the portable exp2 (exp_any is portable in both math modes) and, for F, the rounding of X0 and of the product.
* Scale s_i = F_i / f32(tot_i / P): the relative errors of F, of the sum, and two roundings.  xs = x s: one more.
* Basket: A - 1 roundings of positive partial sums, the rounding of 1 / A and of the product:
  delta_bk = [sum delta_xs + ((1 + U)^(A + 1) - 1) sum (xs + delta_xs)] / A.  max and min are 1-Lipschitz in the
  largest delta_xs of the path.
* Payoff df max(+-(K - u), 0): K rounds to f32 (U K), the difference rounds (U |diff|), max(., 0) is 1-Lipschitz,
  df carries its own error and the product one rounding.
* A mean over the paths moves by the mean of the per-path bounds plus the f64 summation (P 2^-52 relative).
* A standard error sqrt(D / (P (P - 1))), D = sum (v - mean)^2: the centred norm is 1-Lipschitz in the payoff vector,
  so it moves by at most ||delta||_2 / sqrt(P (P - 1)) (at most the largest per-path error over sqrt(P - 1)); the
  kernel forms D as sum v^2 - P m^2 in f64, off by at most H = 4 P 2^-53 sum v^2, and |sqrt(D + H) - sqrt(D)| <=
  sqrt(H).
* The exercise share is a count: a path can be counted differently only if |K - bk| <= delta_bk + U K, so the
  tolerance is the number of such reference paths over P.  exercise_count_ok asks that number to be at most
  max(2, P / 256) for every contract: contracts for which it fails are not used.
* Targets: every output of the DFT is a sum of the N column means with unit-modulus weights: the sum of their
  bounds, plus the f64 transform ((N + 2) 2^-52 sum |mean|) and the rounding of the stored f32 component.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.helpers import math_inputs as mi

U = 2.0 ** -24  # unit roundoff of f32
LU = float(np.log1p(U))
LN2 = float(np.log(2.0))
BLOCK = 8  # contracts simulated at a time by reference()


@dataclass(frozen=True)
class MathEps:
    radius: float  # absolute, of sqrt(-2 ln u1)
    sincos: float  # absolute
    exp2: float    # relative, of the per-step 2^y


PORTABLE = MathEps(mi.RADIUS_MAX_ABS, mi.SINCOS_MAX_ABS, mi.EXP2_MAX_REL)
HW = MathEps(mi.HW_RADIUS_BOUND, max(mi.HW_SIN_BOUND, mi.HW_COS_BOUND), mi.HW_EXP2_BOUND)


def compose(*eps: np.ndarray | float) -> np.ndarray | float:
    """The relative error of a product of factors with these relative errors: prod (1 + e) - 1."""
    out = 1.0
    for e in eps:
        out = out * (1.0 + e)
    return out - 1.0


def fields(rows: np.ndarray, A: int) -> tuple[np.ndarray, ...]:
    """K, T, r, rho [B] and X0, d, v [B, A] of contract rows [B, 3A + 4]."""
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.ndim == 2 and rows.shape[1] == 3 * A + 4
    return (rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4:4 + A], rows[:, 4 + A:4 + 2 * A],
            rows[:, 4 + 2 * A:])


def hand_built_rows(A: int) -> dict[str, np.ndarray]:
    """Contract rows beside the Sobol-drawn ones, by name: d_i and v_i all different in every row, strikes at the
    money (so every payoff is live), rho = 0, the default lower bound max(-0.2, -0.9 / (A - 1)), 0.9, one asset
    without volatility, X0 over four decades within the contract, and at A = 2 the singular corner rho = 1."""
    i = np.arange(A, dtype=np.float64)
    X0, d, v = 80.0 + 10.0 * i, 0.005 * (i + 1.0), 0.15 + 0.07 * i

    def row(rho: float, X0: np.ndarray = X0, v: np.ndarray = v, Tm: float = 1.5) -> np.ndarray:
        return np.concatenate([[X0.mean(), Tm, 0.03, rho], X0, d, v])

    rows = {"rho 0": row(0.0), "rho 0.9": row(0.9, Tm=0.75),
            "one v 0": row(0.3, v=np.where(i == A // 2, 0.0, v)),
            "X0 over four decades": row(0.5, X0=10.0 ** (np.linspace(-1.0, 3.0, A) if A > 1 else np.array([1.0])))}
    if A > 1:
        rows["rho lower bound"] = row(max(-0.2, -0.9 / (A - 1)))
    if A == 2:
        rows["rho 1"] = row(1.0)
    return rows


# ---- drivers -------------------------------------------------------------------------------------------------------
def stream_words(oracle, B: int, A: int, T: int, P: int, seed: int, ordinal0: int) -> np.ndarray:
    """uint32 [B, G, T, 4, pairs, 2]: the words of the G = ceil(P / 4) groups of each contract's stream, in the order
    they are consumed (step, path within the group, pair, (a, b))."""
    pairs, G = (A + 1) // 2, -(-P // 4)
    n = T * 4 * pairs * 2
    w = np.stack([oracle.stream_u32_groups(seed, ordinal0 + b, 0, G, n) for b in range(B)])
    return w.reshape(B, G, T, 4, pairs, 2)


def drivers(words: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(z, radius) [B, 2 pairs, T, 4 G] float64: Box-Muller of every pair, the cosine in slot 2 pair and the sine in
    slot 2 pair + 1, and the radius each came from.  The engine's drivers are the first A slots."""
    B, G, T, four, pairs, two = words.shape
    assert four == 4 and two == 2 and words.dtype == np.uint32
    u1 = 1.0 - (words[..., 0] >> np.uint32(9)).astype(np.float64) * 2.0 ** -23
    angle = 2.0 * np.pi * ((words[..., 1] >> np.uint32(9)).astype(np.float64) * 2.0 ** -23)
    radius = np.sqrt(np.abs(-2.0 * np.log(u1)))  # abs: -2 ln 1 is -0.0
    z = np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=-1)  # [B, G, T, 4, pairs, 2]
    rad = np.stack([radius, radius], axis=-1)

    def by_path(v: np.ndarray) -> np.ndarray:  # -> [B, slot, T, G, 4] -> paths 4 g + j
        return np.ascontiguousarray(v.reshape(B, G, T, 4, 2 * pairs).transpose(0, 4, 2, 1, 3)).reshape(B, 2 * pairs, T, 4 * G)

    return by_path(z), by_path(rad)


def factor(A: int, rho: float) -> np.ndarray:
    """The lower Cholesky factor of the equicorrelation matrix.  At A = 2, rho = 1 (singular, documented as
    meaningful: both assets take the first driver) numpy.linalg.cholesky fails, so that factor is written out."""
    if A == 2 and rho == 1.0:
        return np.array([[1.0, 0.0], [1.0, 0.0]])
    return np.linalg.cholesky((1.0 - rho) * np.eye(A) + rho * np.ones((A, A)))


# ---- paths ---------------------------------------------------------------------------------------------------------
def paths(rows: np.ndarray, A: int, T: int, z: np.ndarray, radius: np.ndarray, eps: MathEps, *,
          L: np.ndarray | None = None, drift: np.ndarray | None = None,
          dt: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(x, rel) [B, A, T, P]: the paths of drivers z [B, A, T, P] and the relative bound of each element.
    L [B, A, A], drift [B, A] (per year) and dt [B] default to the model's: factor(A, rho), r - d - v^2 / 2, T / steps."""
    _, Tm, r, rho, X0, d, v = fields(rows, A)
    assert z.shape[1] == A and z.shape[2] == T and radius.shape == z.shape
    L = np.stack([factor(A, rh) for rh in rho]) if L is None else L
    dt = Tm / T if dt is None else dt
    drift = r[:, None] - d - 0.5 * v * v if drift is None else drift
    vol = v * np.sqrt(dt)[:, None]
    w = np.einsum("bik,bktp->bitp", L, z)
    step = (drift * dt[:, None])[:, :, None, None] + vol[:, :, None, None] * w
    x = X0[:, :, None, None] * np.exp(np.cumsum(step, axis=2))
    # the bound: the kernel's exponent in log2 units
    a = np.abs(drift * dt[:, None]) / LN2
    c = np.abs((vol / LN2)[:, :, None] * L)
    ez = eps.radius + radius * eps.sincos + U * np.abs(z)
    ey = (A + 2) * U * (a[:, :, None, None] + np.einsum("bik,bktp->bitp", c, np.abs(z))) \
        + np.einsum("bik,bktp->bitp", c, ez)
    rel = np.expm1(np.cumsum(LN2 * ey + np.log1p(eps.exp2) + LU, axis=2) + LU)
    return x, rel


def terminal_sums(xT: np.ndarray, relT: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(tot, bound) [B, A] of terminal values [B, A, P]."""
    dx = xT * relT
    tot = xT.sum(axis=-1)
    return tot, dx.sum(axis=-1) + 3 * U * (xT + dx).sum(axis=-1) + xT.shape[-1] * 2.0 ** -52 * tot


# ---- payoffs -------------------------------------------------------------------------------------------------------
def _exp_err(arg: np.ndarray) -> np.ndarray:
    """Relative error of exp_any(f32(g) f32(T)) against e^{g T}, arg = g T."""
    return compose(np.expm1(5 * LU * np.abs(arg)), PORTABLE.exp2)


def forwards(rows: np.ndarray, A: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(F [B, A], its relative bound, df [B], its relative bound)."""
    _, Tm, r, _, X0, d, _ = fields(rows, A)
    g = (r[:, None] - d) * Tm[:, None]
    return X0 * np.exp(g), compose(U, _exp_err(g), U), np.exp(-r * Tm), _exp_err(r * Tm)


def scaled(xT: np.ndarray, relT: np.ndarray, tot: np.ndarray, tot_bound: np.ndarray, normalize: bool,
           F: np.ndarray, eF: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(xs, delta_xs) [B, A, P]: the terminal values on their forwards (NORMALIZE) or as they are (RAW)."""
    if not normalize:
        return xT, xT * relT
    P = xT.shape[-1]
    emean = compose(tot_bound / tot, U, 2.0 ** -52)
    es = (1.0 + eF) * (1.0 + U) / (1.0 - emean) - 1.0
    xs = xT * (F / (tot / P))[:, :, None]
    return xs, xs * compose(relT, es[:, :, None], U)


def _payoff(sign: float, K: np.ndarray, under: np.ndarray, dunder: np.ndarray, df: np.ndarray,
            edf: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """df max(sign (K - under), 0) and its bound; K, df, edf broadcast against under."""
    diff = sign * (K - under)
    u = np.maximum(diff, 0.0)
    du = (U * K + dunder) * (1.0 + U) + U * np.abs(diff)
    return df * u, df * ((u + du) * (1.0 + edf) * (1.0 + U) - u)


def _mean_of(xs: np.ndarray, dxs: np.ndarray, A: int) -> tuple[np.ndarray, np.ndarray]:
    """The equal-weight mean over axis 1 as the kernel forms it (f32 sum in asset order, times f32(1 / A))."""
    S, dS = xs.sum(axis=1), dxs.sum(axis=1)
    return S / A, (dS + ((1.0 + U) ** (A + 1) - 1.0) * (S + dS)) / A


def underlyings(xs: np.ndarray, dxs: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(u, delta_u) [3, B, P]: basket, best and worst of each path."""
    bk, dbk = _mean_of(xs, dxs, xs.shape[1])
    worst = dxs.max(axis=1)
    return np.stack([bk, xs.max(axis=1), xs.min(axis=1)]), np.stack([dbk, worst, worst])


def payoffs(rows: np.ndarray, A: int, u: np.ndarray, du: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(v, delta_v) [2 n, B, P] of underlyings [n, B, P], put then call of each: smc_basket_price's column order for
    underlyings(...)'s basket, best, worst."""
    K = fields(rows, A)[0][:, None]
    _, _, df, edf = forwards(rows, A)
    out = [_payoff(sign, K, u[k], du[k], df[:, None], edf[:, None]) for k in range(u.shape[0]) for sign in (1.0, -1.0)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def price_columns(rows: np.ndarray, A: int, u: np.ndarray, du: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(columns [B, 18], their bounds [B, 18], exercise counts in doubt [B]) from underlyings(...)."""
    K = fields(rows, A)[0]
    B, P = u.shape[1], u.shape[2]
    v, dv = payoffs(rows, A, u, du)
    cols, bound = np.zeros((B, 18)), np.zeros((B, 18))
    cols[:, :6] = v.mean(axis=2).T
    bound[:, :6] = (dv.mean(axis=2) + P * 2.0 ** -52 * v.mean(axis=2)).T
    if P > 1:
        cols[:, 6:12] = (v.std(axis=2, ddof=1) / np.sqrt(P)).T
        H = 4 * P * 2.0 ** -53 * np.square(v + dv).sum(axis=2)
        bound[:, 6:12] = ((np.sqrt(np.square(dv).sum(axis=2)) + np.sqrt(H)) / np.sqrt(P * (P - 1.0))).T
    cols[:, 12:15] = u.mean(axis=2).T
    bound[:, 12:15] = (du.mean(axis=2) + P * 2.0 ** -52 * u.mean(axis=2)).T
    cols[:, 15] = (u[0] < K[:, None]).mean(axis=1)
    doubt = (np.abs(K[:, None] - u[0]) <= du[0] + U * K[:, None]).sum(axis=1)
    bound[:, 15] = doubt / P
    F, eF, df, edf = forwards(rows, A)
    Fb, dFb = _mean_of(F, F * eF, A)
    for col, sign in ((16, 1.0), (17, -1.0)):
        cols[:, col], bound[:, col] = _payoff(sign, K, Fb, dFb, df, edf)
    return cols, bound, doubt


def exercise_count_ok(doubt: np.ndarray, P: int) -> bool:
    """The condition on the contracts a test may use: at most max(2, P / 256) paths of each whose exercise the bound
    leaves open."""
    return bool(np.all(doubt <= max(2, P // 256)))


def targets(put: np.ndarray, dput: np.ndarray, N: int, M: int) -> tuple[np.ndarray, np.ndarray]:
    """(targets [B, N] complex128, bound [B, N] on the real and on the imaginary part) of per-path puts [B, P]."""
    B = put.shape[0]
    avg = put.reshape(B, M, N).mean(axis=1)
    davg = dput.reshape(B, M, N).mean(axis=1) + M * 2.0 ** -52 * avg
    spec = np.fft.fft(avg, axis=1)
    E = davg.sum(axis=1) + (N + 2) * 2.0 ** -52 * np.abs(avg).sum(axis=1)
    return spec, (E[:, None] + U * np.abs(spec)) * (1.0 + U)


# ---- the whole engine ------------------------------------------------------------------------------------------------
@dataclass
class BasketRef:
    x: np.ndarray | None        # [B, A, T, P] stored paths (None unless asked for)
    rel: np.ndarray | None      # their relative bounds
    xT: np.ndarray              # [B, A, P] terminal values
    relT: np.ndarray
    tot: np.ndarray             # [B, A] terminal sums
    tot_bound: np.ndarray
    u: np.ndarray               # [3, B, P] basket, best, worst
    du: np.ndarray
    targets: np.ndarray | None  # [B, N] (None unless N, M given)
    targets_bound: np.ndarray | None
    cols: np.ndarray            # [B, 18]
    cols_bound: np.ndarray
    doubt: np.ndarray           # [B] paths whose exercise the bound leaves open

    @property
    def paths_bound(self) -> np.ndarray:
        return self.x * self.rel


def reference(oracle, rows: np.ndarray, A: int, T: int, P: int, seed: int, ordinal0: int, *, N: int = 0, M: int = 0,
              normalize: bool = True, eps: MathEps = PORTABLE, keep_paths: bool = False) -> BasketRef:
    """Everything the basket kernels produce for these contracts, and its bounds.  P may be any count >= 1 (the
    price call's); N, M (N M = P) add the training targets."""
    rows = np.asarray(rows, dtype=np.float64)
    assert not N or N * M == P
    parts = []
    for b0 in range(0, rows.shape[0], BLOCK):
        blk = rows[b0:b0 + BLOCK]
        z, rad = drivers(stream_words(oracle, blk.shape[0], A, T, P, seed, ordinal0 + b0))
        x, rel = paths(blk, A, T, z[:, :A, :, :P], rad[:, :A, :, :P], eps)
        parts.append(outputs(blk, A, x, rel, N, M, normalize, keep_paths))
    return concat(parts)


def outputs(rows: np.ndarray, A: int, x: np.ndarray, rel: np.ndarray, N: int, M: int, normalize: bool,
            keep_paths: bool = False) -> BasketRef:
    """The engine's outputs downstream of the paths (x, rel) [B, A, T, P]."""
    xT, relT = np.ascontiguousarray(x[:, :, -1, :]), np.ascontiguousarray(rel[:, :, -1, :])
    tot, tot_bound = terminal_sums(xT, relT)
    F, eF, _, _ = forwards(rows, A)
    u, du = underlyings(*scaled(xT, relT, tot, tot_bound, normalize, F, eF))
    cols, cols_bound, doubt = price_columns(rows, A, u, du)
    tg = tb = None
    if N:
        v, dv = payoffs(rows, A, u[:1], du[:1])
        tg, tb = targets(v[0], dv[0], N, M)
    return BasketRef(x if keep_paths else None, rel if keep_paths else None, xT, relT, tot, tot_bound, u, du, tg, tb,
                     cols, cols_bound, doubt)


def concat(parts: list[BasketRef]) -> BasketRef:
    def cat(name: str, axis: int = 0) -> np.ndarray | None:
        vals = [getattr(p, name) for p in parts]
        return None if vals[0] is None else np.concatenate(vals, axis=axis)

    return BasketRef(cat("x"), cat("rel"), cat("xT"), cat("relT"), cat("tot"), cat("tot_bound"), cat("u", 1),
                     cat("du", 1), cat("targets"), cat("targets_bound"), cat("cols"), cat("cols_bound"), cat("doubt"))


def share_used(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> float:
    """The largest |got - want| / bound over the elements (0 / 0 counts as 0, anything / 0 as inf; NaN as inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0.0, 0.0, err / bound)
    share = np.where(np.isnan(share), np.inf, share)
    return float(share.max()) if share.size else 0.0


def complex_share_used(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> float:
    return max(share_used(got.real, want.real, bound), share_used(got.imag, want.imag, bound))
