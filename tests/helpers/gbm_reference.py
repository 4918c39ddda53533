"""An independent float64 reference of the single-asset GBM engine (csrc/gbm.hip: the training kernels, price_kernel
and path_price_kernel), with an a-priori bound on how far the f32 kernels may lie from it, in portable and in
SMC_MATH_HW math; the same for the reference typing (SMC_MATH_REF: rows_ref_kernel) and, evaluated in long double,
for the f64 kernels ("The other typings" below).  numpy only.

What it shares with the kernels: the integer words of the path streams (oracle.stream_u32_groups: Philox pinned by the
Random123 KAT, MWC64X by its Python restatement in tests/test_oracle.py) and the documented meaning of the engine
(csrc/smc_rng.h's header comment, include/spectralmc_hip.h, DESIGN.md sections 3.2f/g).  What it does not share: any
arithmetic.  No log2 units, no folded radius, no per-step exp2, and no call of oracle.kernel_paths, kernel_cf,
kernel_targets, normal_f32_n, exp2_n, gbm_paths, normalize_paths or cf_targets.

The model
---------
Contract row: X0, K, T, r, d, v.  Path p belongs to group p // 4.
Streams: for T >= 3 steps one stream per (seed, ordinal0 + b, group).  For T <= 2 group g takes the (g mod 4)-th run of
4 T words of stream g // 4 (the 16-path stream span).
Draw order: per step pair (t, t + 1), t even, then per path j = 0..3 of the group, one word pair (a, b).  It gives two
standard normals by Box-Muller on u1 = 1 - (a >> 9) 2^-23 in (0, 1] and the angle (b >> 9) 2^-23 revolutions: radius
sqrt(-2 ln u1), the cosine to step t and the sine to step t + 1 of that path.  The last step of an odd T takes two
pairs: pair k feeds paths 2 k (cosine) and 2 k + 1 (sine).  Draws for paths >= P are made and dropped.
Log-Euler:    x_t = X0 exp( sum_{s <= t} [ (r - d - v^2 / 2) dt + v sqrt(dt) z_s ] ),  dt = T / steps.
Simple Euler: x <- | x + x ((r - d) dt + v sqrt(dt) z) |.
Outputs.  NORMALIZE scales row t by F_t / mean_p x_t with the forward F_t = X0 e^{(r - d) t_t} on the grid
linspace(dt, T, steps); RAW leaves the rows as they are.
* the [B, T, P] paths (stored raw under either normalisation) and the [B, T] row sums;
* the training target: numpy.fft.fft of the mean over the M rows of the put df max(K - xs_T, 0) laid out [M, N]
  (path p: row p // N, column p % N), df = e^{-r T}, xs_T the terminal row scaled by F_T / mean x_T;
* the 8 columns of smc_gbm_price: the means of put, call and xs_T, the standard errors sqrt(sample variance / P) of put
  and call (0 at P = 1), the intrinsic values df max(+-(K - F_T), 0), the raw terminal sum;
* the 20 columns of smc_gbm_price_paths on the scaled rows xs_t, monitored at the T grid points (X0 excluded):
  avg = mean_t xs_t, mx = max_t, mn = min_t, knocked = any_t (xs_t <= L or xs_t >= U); the payoffs df max(., 0) of
  K - avg, avg - K, the European pair zeroed when knocked, K - mn, mx - K, K - xs_T, xs_T - K; their means (0..7) and
  standard errors (8..15); the means of avg (16), of the knocked flag (17), of mx (18) and mn (19).  A lower barrier
  <= 0 or an upper one of +inf is switched off.

The bound
---------
Nothing below is fitted to a kernel or to the oracle's kernel mode: the inputs are the reference's own intermediate
values, the f32 unit roundoff U = 2^-24 (or the rounding error of a given input to f32, which the format defines) and
the maximum errors of the device math functions that the sweeps of tests/test_math_accuracy.py (portable) and
tests/test_gpu_math.py (SMC_MATH_HW: twice the measured maxima) assert, by the names of tests/helpers/math_inputs.py
through basket_reference.MathEps: eps_radius, eps_sincos (absolute), eps_exp2 (relative).

A normal z = radius * trig is off by at most
    eps_z = eps_radius + radius eps_sincos + U |z|
(the radius error against a trig value of at most 1, the trig error against the radius, the product's rounding).
Under SMC_MATH_HW the kernel's radius is sqrt(-log2 u1), sqrt(2 ln 2) (kNormalScale) sits in the coefficient b, which
is still one f64 product rounded once to f32, and eps_radius is measured on kNormalScale times the hardware radius:
the same expression holds for b z.

Log-Euler, one step: the kernel's exponent is y = fma(b, z, a) in log2 units, a = drift dt log2 e and
b = v sqrt(dt) log2 e, each computed in f64 and rounded once to f32 (U |a|, U |b z|), and the fma rounds once
(U |y| <= U (|a| + |b z|)).  The HW log-Euler path (hw_log_increments4, hw_log_pair) computes fma(fl(b r), trig, a):
the product b r rounds (U |b z| more) and z itself is never rounded, which eps_z's U |z| term then over-covers.  So
in every instantiation
    eps_y = 3 U (|a| + |b z|) + |b| eps_z,
one U (|a| + |b z|) of which is slack in portable math.  x *= 2^y multiplies the relative error by
e^{ln 2 eps_y} (1 + eps_exp2) (1 + U): the exponent's error, the exp2 kernel, the product's rounding.  An element of a
stored path after t steps lies within the relative bound
    expm1( sum_{s <= t} [ ln 2 eps_y(s) + log1p(eps_exp2) + log1p(U) ] + log1p(U) ),
the last term being the rounding of X0 to f32.

Simple Euler, one step: w = fma(b, z, a) with a = (r - d) dt, b = v sqrt(dt) (times kNormalScale under HW, against
z / kNormalScale), off by delta_w = 3 U (|a| + |b z|) + |b| eps_z as above, and x' = |fma(x, w, x)|.  |.| is
1-Lipschitz, so with an absolute error delta on x
    delta' <= e + U (x' + e),   e = delta |1 + w| + (x + delta) delta_w,
the second term being the rounding of the outer fma.  Where a = b = 0 exactly (no volatility and r = d) the kernel's
w is exactly 0 and fma(x, 0, x) = x is exact: no rounding is charged there.  delta starts at |f32(X0) - X0|.  The
bound is absolute because a reflected path may land arbitrarily close to 0.

Everything after the paths is propagation of absolute errors delta_x (log-Euler: x rel).
* Row sums: the kernel adds a lane's 4 paths in f32 (3 roundings of a partial sum of positive terms) and the rest
  in f64: sum delta_x + 3 U sum (x + delta_x) + P 2^-52 sum x.
* Forward and discount: exp_any(f32(g) f32(t)) = exp2_any of a product of five rounded factors (g, t, their product,
  the f32 constant log2 e, the second product), so e^{g t} carries expm1(5 log1p(U) |g t|), eps_exp2 of the portable
  exp2 (exp_any is portable in both math modes) and, for F, the rounding of X0 and of the product.
* Scale s_t = F_t / f32(rowsum_t / P): the relative errors of F and of the sum, and two roundings.  xs = x s: one more.
* Payoff df max(+-(K - u), 0): K rounds to f32, the difference rounds, max(., 0) is 1-Lipschitz, df carries its own
  error and the product one rounding.
* avg: T - 1 f32 roundings of positive partial sums and the division by T:
  delta_avg = [ sum_t delta_xs + ((1 + U)^T - 1) sum_t (xs + delta_xs) ] / T.  max and min are 1-Lipschitz in the
  largest delta_xs of the path.
* A mean over the paths moves by the mean of the per-path bounds plus the f64 summation (P 2^-52 relative).
* A standard error sqrt(D / (P (P - 1))), D = sum (v - mean)^2: the centred norm is 1-Lipschitz in the payoff vector,
  so it moves by at most ||delta||_2 / sqrt(P (P - 1)); the kernel forms D as sum v^2 - P m^2 in f64, off by at most
  H = 4 P 2^-53 sum v^2, and |sqrt(D + H) - sqrt(D)| <= sqrt(H).
* The knocked flag is a comparison.  With beta = |f32(barrier) - barrier|, a row the reference has outside a barrier
  (xs <= L, say) may be inside for the kernel only if L - xs < delta_xs + beta, and a row inside may be outside only
  if xs - L <= delta_xs + beta.  A path is in doubt if some row of it may flip and no row of it is knocked for sure.
  The knocked share may differ by the number of paths in doubt over P; count_ok asks that number to be at most
  max(2, P / 256) for every contract of a case.  In the knock-out columns a path in doubt may carry its whole European
  payoff as error.
* Targets: every output of the DFT is a sum of the N column means with unit-modulus weights: the sum of their
  bounds, plus the f64 transform ((N + 2) 2^-52 sum |mean|) and the rounding of the stored f32 component.
The float64 errors of the reference itself (1e-15 per operation) are orders below all of this and are left out.

The other typings
-----------------
The unit roundoff and the math maxima are parameters of the propagation above (Typing for the paths, Fmt for what
follows them); F32_PORTABLE / F32_HW give the numbers above bit for bit.  u = 2^-53 below.

The f64 coefficients (Stepper<double>).  drift = (r - d) - v v / 2 rounds three times, each against at most
A = |r - d| + v^2 / 2: 2 u A to first order.  dt = T / steps, drift dt, the constant 256 / ln 2 (kExpUnit) and the
product with it round once each: a is off by at most 6 u A dt.  sqrt(dt) carries half of dt's rounding and its own,
v sqrt(dt), kExpUnit and the last product one each: b is off by at most 4.5 u |b|.  The fma(b, z, a) rounds once
against |a| + |b z|.  Simple Euler has fewer (a: 3, b: 2.5, no constant).  All of it lies within
    8 u (A dt + |b z|),
which is what every f64 step is charged (A dt = |r - d| dt in simple Euler).

Reference typing (rows_ref_kernel, lane_rows_ref; SMC_MATH_REF).  The normal is the f32 one: eps_z as above, in
portable or hardware maxima.  Under SMC_MATH_REF | SMC_MATH_HW normal_pair<true> returns fl(r trig) with the hardware
radius r = sqrt(-log2 u1), and the lane multiplies by kz = f32(sqrt(2 ln 2)): the first product, the rounding of
the constant and the second product are three f32 roundings of |z| where the portable normal has one, and
eps_radius is the hardware one, measured on sqrt(2 ln 2) r:
    eps_z = eps_radius + radius eps_sincos + n_z U |z|,   n_z = 1 (portable), 3 (hardware).
z widens to f64 exactly.  Log-Euler: y = fma(b, z, a) in units of ln 2 / 256, so in natural units
    eps_y = v sqrt(dt) eps_z + 8 u (A dt + |b z|),
and x <- mul_exp2s_f64(x, y), which tests/test_math_accuracy.py and tests/test_oracle.py hold within 2 ulp; one ulp
more is charged for the libm those tests compare with: 3 ulp <= 6 u relative per step, the product's rounding
included.  The state stays in f64 from step to step; a stored element is the state rounded once to f32, and X0
enters as the f64 it is:
    expm1( sum_{s <= t} [ eps_y(s) + log1p(6 u) ] + log1p(U) ).
Simple Euler: delta_w = v sqrt(dt) eps_z + 8 u (|a| + |b z|), the recursion above with u for the outer fma's
rounding and delta = 0 at the start, and a stored element carries U (x + delta) more (|f32(X0) - X0| where
a = b = 0 keeps the state on X0).  What follows the paths is the f32 pipeline on the stored f32 rows: the lane adds
its four rounded terminal values in f32 and cf_kernel<float> reads the stored row, so outputs() applies unchanged.

f64 engine (every Real = double kernel).  The uniforms are u1 = (a + 1/2) 2^-32 and the angle of all 32 bits of b
(math_inputs.sincos_u32_angle_units 2^-32 turns).  The reference is evaluated in numpy.longdouble (64-bit
significand: LONGDOUBLE_OK), pi from a long-double literal: its own error is of the 2^-64 class, three orders below
the bound, and is left out.  m2log_u32 is within 2 ulp of libm (tests/test_oracle.py
test_f64_uniform_transcendentals_are_accurate), libm is charged 1 ulp: 6 u relative on -2 ln u1, 3 u on its root,
sqrt_radius rounds correctly (u more), and the product with the trig value (box_muller) or with b
(f64_log_increments4 / f64_log_tail4, which fold b into the radius and never round z itself) once more; sin and cos
are within 2^-52 absolute:
    eps_z = radius 2^-52 + 5 u |z|.
The step is the reference typing's with this eps_z, no f32 store and X0 exact:
    expm1( sum_{s <= t} [ v sqrt(dt) eps_z + 8 u (A dt + |b z|) + log1p(6 u) ] ).
oracle.gbm_paths(dtype="float64") is held to the same bound although it takes libm's exp in natural units: its
exponent drift dt + v (z sqrt(dt)) has no kExpUnit products (fewer roundings than the 8 charged), and libm's exp
(1 ulp) times x (one rounding) is 3 u against the 6 u charged.  Its simple-Euler step X += (r - d) X dt + v X dW
rounds w's terms about 6.5 times against |a| + |b z| and the sum once against x': within the same recursion.
Downstream is the propagation above with U = u: the f64 kernels are the f32 ones with Real = double (the lane's four
values added in Real, s = F / Real(sum / P), xs = x s, Payoff<double>).  Given inputs are f64 already and do not
round.  e^{g t} is the device exp of an f64 product: g = r - d, the product and, in normalize_kernel and
path_price_kernel, the grid point dt + t (T - dt) / (steps - 1) (five roundings to first order) make at most 8
rounded factors, and the exp itself is charged 2 ulp = 4 u (the documented maximum of the device and host libm exp
is 1 ulp).  The f64 accumulations (P 2^-52 and the like) are the terms that now dominate.  One term is sharper than in
f32: max(., 0) is 1-Lipschitz, but a path out of the money by more than the bound of its difference pays exactly 0 in
the kernel as well, so it is charged max(diff + du, 0) and not du.  (In f32 the plain du stands, as it always has; it
is the larger one.)  Without it a far out-of-the-money path of a high-volatility simple-Euler contract would carry the
absolute bound of a value 10^7 times the strike into a put that is certainly zero.

The keyword arguments marked "wrong reading" exist for the sensitivity tests of tests/test_gbm_reference.py and
tests/test_gbm_typing_reference.py only.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests.helpers.basket_reference import HW, PORTABLE, MathEps, complex_share_used, compose, share_used
from tests.helpers.math_inputs import sincos_turns_longdouble, sincos_u32_angle_units

__all__ = ["HW", "PORTABLE", "MathEps", "complex_share_used", "compose", "share_used"]

U = 2.0 ** -24  # unit roundoff of f32
U64 = 2.0 ** -53  # unit roundoff of f64
LU = float(np.log1p(U))
LN2 = float(np.log(2.0))
LOG_EULER, SIMPLE_EULER = 0, 1
ELEMENTS = 1 << 22  # path elements simulated at a time by reference()
NORMAL_SCALE = float(np.sqrt(2.0 * np.log(2.0)))  # kNormalScale<true> of csrc/smc_rng.h
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63  # the f64 engine's reference needs a 64-bit significand


@dataclass(frozen=True)
class Fmt:
    """The number format of a kernel's stored rows and of everything after them."""
    u: float            # unit roundoff
    exp_factors: int    # rounded factors in the argument of e^{g t}
    exp_eps: float      # relative error of the exponential itself
    inputs_round: bool  # a given f64 input (X0, K, a barrier) is rounded to the format
    sharp_payoff: bool  # a payoff out of the money by more than its bound is charged what is left of the bound only
    real: type          # what the reference is evaluated in

    @property
    def lu(self) -> float:
        return float(np.log1p(self.u))

    def input_error(self, x: np.ndarray) -> np.ndarray:
        return f32_error(x) if self.inputs_round else np.zeros(np.shape(x))


F32 = Fmt(U, 5, PORTABLE.exp2, True, False, np.float64)
F64 = Fmt(U64, 8, 4 * U64, False, True, np.longdouble)


@dataclass(frozen=True)
class Typing:
    """How a kernel types its path recursion: what the path bound needs of it (the module docstring derives each)."""
    eps: MathEps      # maxima of the normal's radius and trig value (absolute) and of the step's exponential (relative)
    nz: int           # roundings of |z| itself ...
    uz: float         # ... in the normal's format
    nc: int           # roundings charged to the step's coefficients and fma ...
    uc: float         # ... in their format
    f64_coef: bool    # the coefficients are formed and kept in f64: charged against (|r - d| + v^2 / 2) dt, not |a|
    ustep: tuple[float, float]  # rounding of the state in a step beside eps.exp2: (log-Euler: the product,
                      # simple Euler: the outer fma)
    x0_rounds: bool   # X0 is rounded to f32 on entry
    ustore: float     # rounding of a stored element that the state does not carry
    fmt: Fmt          # the stored rows and what follows them
    f64_normals: bool = False  # the f64 engine's uniforms, evaluated in long double


def f32_typing(eps: MathEps) -> Typing:
    return Typing(eps, 1, U, 3, U, False, (U, U), True, 0.0, F32)


def ref_typing(eps: MathEps) -> Typing:
    """SMC_MATH_REF on the portable (eps = PORTABLE) or the hardware (HW) f32 normals."""
    return Typing(MathEps(eps.radius, eps.sincos, 6 * U64), 3 if eps is HW else 1, U, 8, U64, True, (0.0, U64),
                  False, U, F32)


F32_PORTABLE, F32_HW = f32_typing(PORTABLE), f32_typing(HW)
REF_PORTABLE, REF_HW = ref_typing(PORTABLE), ref_typing(HW)
F64_ENGINE = Typing(MathEps(0.0, 2.0 ** -52, 6 * U64), 5, U64, 8, U64, True, (0.0, U64), False, 0.0, F64, True)


def fields(rows: np.ndarray) -> tuple[np.ndarray, ...]:
    """X0, K, T, r, d, v [B] of contract rows [B, 6]."""
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.ndim == 2 and rows.shape[1] == 6
    return tuple(rows[:, k] for k in range(6))


def f32_error(x: np.ndarray) -> np.ndarray:
    """|f32(x) - x|: what rounding a given input to f32 costs."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isfinite(x), np.abs(x.astype(np.float32).astype(np.float64) - x), 0.0)


# Hand-built contracts beside the Sobol-drawn ones, by name.  "flat" (no volatility, r = d, X0 a f32 number) keeps
# every simple-Euler path on X0 exactly, with a zero bound: a barrier placed on X0 then tells <= from < (hand_built_
# barriers).  "reflected" steps over zero in simple Euler on about every other draw.  "low forward" (r - d < 0 over a
# long maturity) keeps the average, maximum and minimum far from X0.
HAND_BUILT = {
    "v 0": (100.0, 95.0, 2.0, 0.05, 0.01, 0.0),
    "T v^2 corner": (100.0, 100.0, 10.0, 0.03, 0.01, 2.0),
    "deep in the money": (100.0, 400.0, 1.0, 0.03, 0.0, 0.2),
    "deep out of the money": (100.0, 25.0, 1.0, 0.03, 0.0, 0.2),
    "X0 0.1": (0.1, 0.11, 1.5, 0.02, 0.01, 0.3),
    "X0 1000": (1000.0, 900.0, 0.75, 0.04, 0.0, 0.25),
    "low forward": (100.0, 80.0, 5.0, -0.05, 0.1, 0.15),
    "flat": (128.0, 128.0, 1.0, 0.03, 0.03, 0.0),
    "reflected": (100.0, 100.0, 9.0, 0.01, 0.0, 1.8),
}


def hand_built_rows() -> np.ndarray:
    return np.array(list(HAND_BUILT.values()), dtype=np.float64)


def default_barriers(rows: np.ndarray) -> np.ndarray:
    """[B, 2] (lower, upper): L = X0 exp(-v sqrt(T)), U = max(X0, F) exp(v sqrt(T)), about one standard deviation out."""
    X0, _, Tm, r, d, v = fields(rows)
    F = X0 * np.exp((r - d) * Tm)
    return np.stack([X0 * np.exp(-v * np.sqrt(Tm)), np.maximum(X0, F) * np.exp(v * np.sqrt(Tm))], axis=1)


def hand_built_barriers(scheme: int, normalize: bool) -> np.ndarray:
    """Barriers of hand_built_rows(): the default ones, except that "v 0" gets barriers well off its forward curve,
    "X0 1000" an upper barrier inside the bulk (at its forward) and "flat" an upper barrier on X0 itself where the
    bound is zero (simple Euler, RAW), well off it elsewhere."""
    rows = hand_built_rows()
    bars = default_barriers(rows)
    names = list(HAND_BUILT)
    bars[names.index("v 0")] = (50.0, 200.0)
    i = names.index("X0 1000")
    bars[i, 1] = rows[i, 0] * np.exp((rows[i, 3] - rows[i, 4]) * rows[i, 2])
    bars[names.index("flat")] = (64.0, 128.0 if scheme == SIMPLE_EULER and not normalize else 256.0)
    return bars


# ---- normals ---------------------------------------------------------------------------------------------------------
def stream_words(oracle, B: int, T: int, P: int, seed: int, ordinal0: int, *, span: bool = True) -> np.ndarray:
    """uint32 [B, G, 4 T]: the words group g = 0 .. ceil(P / 4) - 1 of each contract consumes, in order.
    span = False (wrong reading): one stream per group at T <= 2 as well."""
    G, n = -(-P // 4), 4 * T
    if T <= 2 and span:
        S = -(-G // 4)
        w = np.stack([oracle.stream_u32_groups(seed, ordinal0 + b, 0, S, 4 * n) for b in range(B)])
        return np.ascontiguousarray(w.reshape(B, 4 * S, n)[:, :G])
    return np.stack([oracle.stream_u32_groups(seed, ordinal0 + b, 0, G, n) for b in range(B)])


def normals(words: np.ndarray, T: int, P: int, *, exchange: bool = False, tail_stride: bool = False,
            complement: bool = True, f64: bool = False, longdouble: bool = False,
            plain_angle: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """(z, radius) [B, T, P] float64 of stream_words(...).  Wrong readings: exchange (the sine to step t, the cosine to
    t + 1), tail_stride (pair k of the odd tail to paths k and k + 2), complement = False (u1 = (a >> 9) 2^-23).
    f64: the uniforms of the float64 engine, in the same draw order: u1 = (a + 1/2) 2^-32 and the angle of all 32
    bits of b (math_inputs.sincos_u32_angle_units 2^-32 revolutions); longdouble: those evaluated in numpy.longdouble
    (the angle reduced exactly to the nearest quarter turn, pi from a long-double literal: math_inputs.
    sincos_turns_longdouble); plain_angle (wrong reading, with longdouble): the angle b 2^-32 revolutions."""
    B, G, n = words.shape
    assert n == 4 * T and words.dtype == np.uint32
    assert f64 or not (longdouble or plain_angle)
    trig = None
    if longdouble:
        u1 = (words[..., 0::2].astype(np.longdouble) + np.longdouble(0.5)) * np.longdouble(2.0 ** -32)
        units = words[..., 1::2].astype(np.int64) if plain_angle else sincos_u32_angle_units(words[..., 1::2])
        trig = sincos_turns_longdouble(units, 32)
    elif f64:
        u1 = (words[..., 0::2].astype(np.float64) + 0.5) * 2.0 ** -32
        angle = 2.0 * np.pi * (sincos_u32_angle_units(words[..., 1::2]).astype(np.float64) * 2.0 ** -32)
    else:
        m = (words[..., 0::2] >> np.uint32(9)).astype(np.float64) * 2.0 ** -23
        u1 = 1.0 - m if complement else m
        angle = 2.0 * np.pi * ((words[..., 1::2] >> np.uint32(9)).astype(np.float64) * 2.0 ** -23)
    with np.errstate(divide="ignore", invalid="ignore"):
        radius = np.sqrt(np.abs(-2.0 * np.log(u1)))  # abs: -2 ln 1 is -0.0; [B, G, 2 T]
        sin, cos = trig if trig is not None else (np.sin(angle), np.cos(angle))
        first, second = radius * cos, radius * sin
    if exchange:
        first, second = second, first
    z = np.empty((B, T, G, 4), dtype=radius.dtype)
    rad = np.empty((B, T, G, 4), dtype=radius.dtype)
    H = T // 2
    if H:  # pair index (step pair h, path j) -> steps 2 h, 2 h + 1 of path j
        for out, a, b in ((z, first, second), (rad, radius, radius)):
            out[:, 0:2 * H:2] = a[..., :4 * H].reshape(B, G, H, 4).transpose(0, 2, 1, 3)
            out[:, 1:2 * H:2] = b[..., :4 * H].reshape(B, G, H, 4).transpose(0, 2, 1, 3)
    if T % 2:
        for out, a, b in ((z, first, second), (rad, radius, radius)):
            ta, tb = a[..., 4 * H:], b[..., 4 * H:]  # [B, G, 2]: pair k
            quad = np.stack([ta[..., 0], ta[..., 1], tb[..., 0], tb[..., 1]] if tail_stride else
                            [ta[..., 0], tb[..., 0], ta[..., 1], tb[..., 1]], axis=-1)
            out[:, T - 1] = quad
    return (np.ascontiguousarray(z.reshape(B, T, 4 * G)[:, :, :P]),
            np.ascontiguousarray(rad.reshape(B, T, 4 * G)[:, :, :P]))


# ---- paths -----------------------------------------------------------------------------------------------------------
def _f32(x: np.ndarray) -> np.ndarray:
    return x.astype(np.float32).astype(x.dtype)


def paths(rows: np.ndarray, T: int, z: np.ndarray, radius: np.ndarray, eps: MathEps | Typing,
          scheme: int = LOG_EULER, *, drift: np.ndarray | None = None, dt: np.ndarray | None = None,
          reflect: bool = True, round_state: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """(x, delta_x) [B, T, P]: the paths of normals z [B, T, P], in z's dtype, and the absolute bound of each stored
    element.  eps: the typing of the kernel, or the math maxima of an f32 one.
    drift [B] (per year; log-Euler r - d - v^2 / 2, simple Euler r - d) and dt [B] default to the model's;
    reflect = False (wrong reading): simple Euler without the absolute value; round_state (wrong reading): the state
    rounded to f32 after every step."""
    ty = eps if isinstance(eps, Typing) else f32_typing(eps)
    eps = ty.eps
    X0, _, Tm, r, d, v = (f.astype(z.dtype) for f in fields(rows))
    assert z.shape[:2] == (rows.shape[0], T) and radius.shape == z.shape
    dt = Tm / T if dt is None else dt
    vol = (v * np.sqrt(dt))[:, None, None]
    ez = eps.radius + radius * eps.sincos + ty.nz * ty.uz * np.abs(z)
    once = (LU if ty.x0_rounds else 0.0) + float(np.log1p(ty.ustore))
    if scheme == LOG_EULER:
        drift = r - d - 0.5 * v * v if drift is None else drift
        a = (drift * dt)[:, None, None]
        amag = ((np.abs(r - d) + 0.5 * v * v) * dt)[:, None, None] if ty.f64_coef else np.abs(a)
        if round_state:
            x = np.empty_like(z)
            cur = np.broadcast_to(X0[:, None], z[:, 0].shape)
            for t in range(T):
                cur = _f32(cur * np.exp(a[:, 0] + vol[:, 0] * z[:, t]))
                x[:, t] = cur
        else:
            x = X0[:, None, None] * np.exp(np.cumsum(a + vol * z, axis=1))
        ey = ty.nc * ty.uc * (amag + np.abs(vol * z)) / LN2 + vol / LN2 * ez  # in log2 units
        rel = np.expm1(np.cumsum(LN2 * ey + np.log1p(eps.exp2) + float(np.log1p(ty.ustep[0])), axis=1) + once)
        return x, x * rel
    assert scheme == SIMPLE_EULER
    drift = r - d if drift is None else drift
    a = (drift * dt)[:, None]
    w = a[:, :, None] + vol * z
    dw = ty.nc * ty.uc * (np.abs(a[:, :, None]) + np.abs(vol * z)) + vol * ez
    exact = ((a == 0.0) & (vol[:, :, 0] == 0.0))  # [B, 1]: every step of the contract is fma(x, 0, x) = x
    x, dx = np.empty_like(z), np.empty_like(z)
    cur = np.broadcast_to(X0[:, None], z[:, 0].shape)
    dcur = np.broadcast_to((f32_error(X0) if ty.x0_rounds else np.zeros_like(X0))[:, None], cur.shape)
    for t in range(T):
        nxt = cur * (1.0 + w[:, t])
        nxt = np.abs(nxt) if reflect else nxt
        nxt = _f32(nxt) if round_state else nxt
        e = dcur * np.abs(1.0 + w[:, t]) + (cur + dcur) * dw[:, t]
        dcur = e + np.where(exact, 0.0, ty.ustep[1]) * (np.abs(nxt) + e)
        cur = nxt
        x[:, t], dx[:, t] = cur, dcur
        if ty.ustore:  # the store rounds a state that stays unrounded
            dx[:, t] = dcur + np.where(exact, f32_error(cur), ty.ustore * (np.abs(cur) + dcur))
    return x, dx


def row_sums(x: np.ndarray, dx: np.ndarray, *, fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """(sum over the paths, its bound) along the last axis."""
    tot = x.sum(axis=-1)
    return tot, (dx.sum(axis=-1) + 3 * fmt.u * (np.abs(x) + dx).sum(axis=-1)
                 + x.shape[-1] * 2.0 ** -52 * np.abs(x).sum(axis=-1))


# ---- payoffs ---------------------------------------------------------------------------------------------------------
def exp_err(arg: np.ndarray, *, fmt: Fmt = F32) -> np.ndarray:
    """Relative error of the kernel's e^{g t} (f32: exp_any(f32(g) f32(t))) against the true one, arg = g t."""
    return compose(np.expm1(fmt.exp_factors * fmt.lu * np.abs(arg)), fmt.exp_eps)


def forwards(rows: np.ndarray, T: int, *, early: bool = False, fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """(F [B, T], its relative bound) on the grid linspace(dt, T, steps).  early (wrong reading): row t at t dt."""
    X0, _, Tm, r, d, _ = (f.astype(fmt.real) for f in fields(rows))
    if fmt.real is np.float64:
        grid = np.stack([np.linspace(tm / T, tm, T) for tm in Tm])
    else:
        grid = Tm[:, None] * np.arange(1, T + 1).astype(fmt.real) / T
    if early:
        grid = grid - (Tm / T)[:, None]
    g = (r - d)[:, None] * grid
    return X0[:, None] * np.exp(g), compose(fmt.u, exp_err(g, fmt=fmt), fmt.u)


def discount(rows: np.ndarray, *, carry: bool = False, fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """(df [B], its relative bound).  carry (wrong reading): e^{-(r - d) T}."""
    _, _, Tm, r, d, _ = (f.astype(fmt.real) for f in fields(rows))
    g = (r - d if carry else r) * Tm
    return np.exp(-g), exp_err(g, fmt=fmt)


def scaled(x: np.ndarray, dx: np.ndarray, tot: np.ndarray, tot_bound: np.ndarray, F: np.ndarray,
           eF: np.ndarray, *, fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """(xs, delta_xs): rows x [..., P] on their forwards F [...] given their sums."""
    P, u = x.shape[-1], fmt.u
    emean = compose(tot_bound / tot, u, 2.0 ** -52)
    es = ((1.0 + eF) * (1.0 + u) / (1.0 - emean) - 1.0)[..., None]
    s = (F / (tot / P))[..., None]
    xs = x * s
    return xs, (dx * s) * (1.0 + es) * (1.0 + u) + np.abs(xs) * compose(es, u)


def payoff(sign: float, K: np.ndarray, under: np.ndarray, dunder: np.ndarray, df: np.ndarray,
           edf: np.ndarray, *, fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """df max(sign (K - under), 0) and its bound; K, df, edf broadcast against under."""
    diff = sign * (K - under)
    u = np.maximum(diff, 0.0)
    du = (fmt.input_error(K) + dunder) * (1.0 + fmt.u) + fmt.u * np.abs(diff)
    if fmt.sharp_payoff:  # the kernel's difference is below diff + du: where that is negative its payoff is 0 as well
        du = np.where(diff < 0.0, np.maximum(diff + du, 0.0), du)
    return df * u, df * ((u + du) * (1.0 + edf) * (1.0 + fmt.u) - u)


def mean_and_stderr(v: np.ndarray, dv: np.ndarray) -> tuple[np.ndarray, ...]:
    """(mean, its bound, standard error, its bound) over the last axis of per-path values and bounds."""
    P = v.shape[-1]
    m = v.mean(axis=-1)
    dm = dv.mean(axis=-1) + P * 2.0 ** -52 * np.abs(v).mean(axis=-1)
    if P == 1:
        return m, dm, np.zeros_like(m), np.zeros_like(m)
    se = v.std(axis=-1, ddof=1) / np.sqrt(P)
    H = 4 * P * 2.0 ** -53 * np.square(np.abs(v) + dv).sum(axis=-1)
    return m, dm, se, (np.sqrt(np.square(dv).sum(axis=-1)) + np.sqrt(H)) / np.sqrt(P * (P - 1.0))


def price_columns(rows: np.ndarray, xs: np.ndarray, dxs: np.ndarray, FT: np.ndarray, eFT: np.ndarray,
                  tot: np.ndarray, tot_bound: np.ndarray, *, carry: bool = False,
                  fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """(columns [B, 8], their bounds) of smc_gbm_price from the scaled terminal values xs [B, P], the terminal forward
    and the raw terminal sum."""
    K = fields(rows)[1].astype(fmt.real)
    df, edf = discount(rows, carry=carry, fmt=fmt)
    B = xs.shape[0]
    cols, bound = np.zeros((B, 8), dtype=fmt.real), np.zeros((B, 8), dtype=fmt.real)
    for k, sign in ((0, 1.0), (1, -1.0)):
        v, dv = payoff(sign, K[:, None], xs, dxs, df[:, None], edf[:, None], fmt=fmt)
        cols[:, k], bound[:, k], cols[:, 3 + k], bound[:, 3 + k] = mean_and_stderr(v, dv)
        cols[:, 5 + k], bound[:, 5 + k] = payoff(sign, K, FT, FT * eFT, df, edf, fmt=fmt)
    cols[:, 2], bound[:, 2], _, _ = mean_and_stderr(xs, dxs)
    cols[:, 7], bound[:, 7] = tot, tot_bound
    return cols, bound


def _flips(xs: np.ndarray, dxs: np.ndarray, bars: np.ndarray, strict: bool,
           fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """(knocked [B, P], in doubt [B, P]) of rows xs [B, T, P] and barriers [B, 2]."""
    lower, upper = bars[:, 0, None, None], bars[:, 1, None, None]
    lo_on, up_on = lower > 0.0, np.isfinite(upper)
    bl, bu = fmt.input_error(bars[:, 0])[:, None, None], fmt.input_error(bars[:, 1])[:, None, None]
    with np.errstate(invalid="ignore"):
        out_lo = lo_on & ((xs < lower) if strict else (xs <= lower))
        out_up = up_on & ((xs > upper) if strict else (xs >= upper))
        gap_lo, gap_up = np.where(lo_on, xs - lower, np.inf), np.where(up_on, upper - xs, np.inf)
    # a row outside may be inside for the kernel if -gap < delta + beta; a row inside may be outside if gap <= delta + beta
    flip = np.where(out_lo, -gap_lo < dxs + bl, gap_lo <= dxs + bl) | np.where(out_up, -gap_up < dxs + bu, gap_up <= dxs + bu)
    sure = ((out_lo & ~(-gap_lo < dxs + bl)) | (out_up & ~(-gap_up < dxs + bu))).any(axis=1)
    return (out_lo | out_up).any(axis=1), flip.any(axis=1) & ~sure


def path_columns(rows: np.ndarray, bars: np.ndarray, xs: np.ndarray, dxs: np.ndarray, *, strict: bool = False,
                 with_x0: bool = False, carry: bool = False,
                 fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(columns [B, 20], their bounds, knocked flags in doubt [B]) of smc_gbm_price_paths from the scaled rows
    xs [B, T, P].  Wrong readings: strict barrier comparisons; with_x0: X0 monitored as well."""
    X0, K = (f.astype(fmt.real) for f in fields(rows)[:2])
    df, edf = discount(rows, carry=carry, fmt=fmt)
    B, T, P = xs.shape
    mon, dmon = xs, dxs
    if with_x0:
        mon = np.concatenate([np.broadcast_to(X0[:, None, None], (B, 1, P)), xs], axis=1)
        dmon = np.concatenate([np.zeros((B, 1, P), dtype=dxs.dtype), dxs], axis=1)
    n = mon.shape[1]
    S, dS = mon.sum(axis=1), dmon.sum(axis=1)
    avg, davg = S / n, (dS + ((1.0 + fmt.u) ** n - 1.0) * (S + dS)) / n
    worst = dmon.max(axis=1)
    mx, mn = mon.max(axis=1), mon.min(axis=1)
    ko, doubt = _flips(xs, dxs, np.asarray(bars, dtype=np.float64), strict, fmt)
    Kc, dfc, edfc = K[:, None], df[:, None], edf[:, None]
    pay = functools.partial(payoff, fmt=fmt)
    eur = [pay(sign, Kc, xs[:, -1], dxs[:, -1], dfc, edfc) for sign in (1.0, -1.0)]
    # a path in doubt may be paid in full or not at all
    kos = [(np.where(ko, 0.0, v), np.where(doubt, v + dv, np.where(ko, 0.0, dv))) for v, dv in eur]
    pays = [pay(1.0, Kc, avg, davg, dfc, edfc), pay(-1.0, Kc, avg, davg, dfc, edfc), kos[0], kos[1],
            pay(1.0, Kc, mn, worst, dfc, edfc), pay(-1.0, Kc, mx, worst, dfc, edfc), eur[0], eur[1]]
    cols, bound = np.zeros((B, 20), dtype=fmt.real), np.zeros((B, 20), dtype=fmt.real)
    for k, (v, dv) in enumerate(pays):
        cols[:, k], bound[:, k], cols[:, 8 + k], bound[:, 8 + k] = mean_and_stderr(v, dv)
    for col, (v, dv) in ((16, (avg, davg)), (18, (mx, worst)), (19, (mn, worst))):
        cols[:, col], bound[:, col], _, _ = mean_and_stderr(v, dv)
    cols[:, 17], bound[:, 17] = ko.mean(axis=1), doubt.sum(axis=1) / P
    return cols, bound, doubt.sum(axis=1)


def count_ok(doubt: np.ndarray, P: int) -> bool:
    """The condition on the barriers a test may use: at most max(2, P / 256) paths of each contract whose knocked flag
    the bound leaves open."""
    return bool(np.all(doubt <= max(2, P // 256)))


def targets(put: np.ndarray, dput: np.ndarray, N: int, M: int, *, transposed: bool = False,
            fmt: Fmt = F32) -> tuple[np.ndarray, np.ndarray]:
    """(targets [B, N] complex128, bound [B, N] on the real and on the imaginary part) of per-path puts [B, P].
    transposed (wrong reading): path p in row p % M, column p // M."""
    B = put.shape[0]
    lay = (lambda a: a.reshape(B, N, M).transpose(0, 2, 1)) if transposed else (lambda a: a.reshape(B, M, N))
    avg = lay(put).mean(axis=1)
    davg = lay(dput).mean(axis=1) + M * 2.0 ** -52 * avg
    spec = np.fft.fft(avg, axis=1)
    E = davg.sum(axis=1) + (N + 2) * 2.0 ** -52 * np.abs(avg).sum(axis=1)
    return spec, (E[:, None] + fmt.u * np.abs(spec)) * (1.0 + fmt.u)


# ---- the whole engine ------------------------------------------------------------------------------------------------
@dataclass
class GbmRef:
    x: np.ndarray | None        # [B, T, P] raw paths (None unless asked for)
    dx: np.ndarray | None       # their absolute bounds
    xT: np.ndarray              # [B, P] raw terminal values
    dxT: np.ndarray
    rowsum: np.ndarray          # [B, T] raw row sums
    rowsum_bound: np.ndarray
    targets: np.ndarray | None  # [B, N] (None unless N, M given)
    targets_bound: np.ndarray | None
    price: np.ndarray           # [B, 8]
    price_bound: np.ndarray
    path: np.ndarray | None     # [B, 20] (None unless barriers given)
    path_bound: np.ndarray | None
    doubt: np.ndarray | None    # [B] paths whose knocked flag the bound leaves open


def outputs(rows: np.ndarray, x: np.ndarray, dx: np.ndarray, *, N: int = 0, M: int = 0, normalize: bool = True,
            bars: np.ndarray | None = None, keep_paths: bool = False, early: bool = False, transposed: bool = False,
            strict: bool = False, with_x0: bool = False, carry: bool = False, fmt: Fmt = F32) -> GbmRef:
    """The engine's outputs downstream of the stored raw paths (x, delta_x) [B, T, P], computed in the format fmt."""
    T = x.shape[1]
    rs, rsb = row_sums(x, dx, fmt=fmt)
    F, eF = forwards(rows, T, early=early, fmt=fmt)
    if normalize:
        if bars is not None:
            xs, dxs = scaled(x, dx, rs, rsb, F, eF, fmt=fmt)
            xsT, dxsT = xs[:, -1], dxs[:, -1]
        else:
            xsT, dxsT = scaled(x[:, -1], dx[:, -1], rs[:, -1], rsb[:, -1], F[:, -1], eF[:, -1], fmt=fmt)
    else:
        xs, dxs, xsT, dxsT = x, dx, x[:, -1], dx[:, -1]
    price, price_bound = price_columns(rows, xsT, dxsT, F[:, -1], eF[:, -1], rs[:, -1], rsb[:, -1], carry=carry,
                                       fmt=fmt)
    path = path_bound = doubt = tg = tb = None
    if bars is not None:
        path, path_bound, doubt = path_columns(rows, bars, xs, dxs, strict=strict, with_x0=with_x0, carry=carry,
                                               fmt=fmt)
    if N:
        df, edf = discount(rows, carry=carry, fmt=fmt)
        K = fields(rows)[1].astype(fmt.real)
        put, dput = payoff(1.0, K[:, None], xsT, dxsT, df[:, None], edf[:, None], fmt=fmt)
        tg, tb = targets(put, dput, N, M, transposed=transposed, fmt=fmt)
    xT, dxT = np.ascontiguousarray(x[:, -1]), np.ascontiguousarray(dx[:, -1])
    return GbmRef(x if keep_paths else None, dx if keep_paths else None, xT, dxT, rs, rsb, tg, tb, price, price_bound,
                  path, path_bound, doubt)


def concat(parts: list[GbmRef]) -> GbmRef:
    def cat(name: str) -> np.ndarray | None:
        vals = [getattr(p, name) for p in parts]
        return None if vals[0] is None else np.concatenate(vals, axis=0)

    return GbmRef(*(cat(name) for name in GbmRef.__dataclass_fields__))


def reference(oracle, rows: np.ndarray, T: int, P: int, seed: int, ordinal0: int, *, scheme: int = LOG_EULER,
              eps: MathEps | Typing = PORTABLE, N: int = 0, M: int = 0, normalize: bool = True,
              bars: np.ndarray | None = None, keep_paths: bool = False) -> GbmRef:
    """Everything the single-asset kernels produce for these contracts, and its bounds.  P may be any count >= 1;
    N, M (N M = P) add the training targets, bars [B, 2] the 20 columns of smc_gbm_price_paths.  eps: the kernel's
    typing (F32_PORTABLE, F32_HW, REF_PORTABLE, REF_HW, F64_ENGINE), or the math maxima of an f32 kernel."""
    ty = eps if isinstance(eps, Typing) else f32_typing(eps)
    assert LONGDOUBLE_OK or not ty.f64_normals
    rows = np.asarray(rows, dtype=np.float64)
    assert not N or N * M == P
    block = max(1, ELEMENTS // (T * P))
    parts = []
    for b0 in range(0, rows.shape[0], block):
        blk = rows[b0:b0 + block]
        z, rad = normals(stream_words(oracle, blk.shape[0], T, P, seed, ordinal0 + b0), T, P, f64=ty.f64_normals,
                         longdouble=ty.f64_normals)
        x, dx = paths(blk, T, z, rad, ty, scheme)
        parts.append(outputs(blk, x, dx, N=N, M=M, normalize=normalize, bars=None if bars is None else bars[b0:b0 + block],
                             keep_paths=keep_paths, fmt=ty.fmt))
    return concat(parts)
