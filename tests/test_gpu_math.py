"""The device math functions (csrc/smc_math.h, the Box-Muller of csrc/smc_rng.h) through the test hook
smc_test_math_eval, swept over their whole input domains: the portable f32 and the f64 functions against the
oracle's restatement bit for bit, sqrt_radius against the correctly rounded root, and the SMC_MATH_HW
hardware-transcendental arithmetic against f64 references of its exact inputs.  tests/test_math_accuracy.py bounds
the restatement's own error over the same inputs, so the two files together bound the device functions' error.

Every call is one launch (two where n would otherwise fill its last workgroup) into a NaN-poisoned buffer with a
poisoned guard behind it."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from spectralmc_amd import _lib
from tests.helpers import assert_rows_equal, poisoned
from tests.helpers import math_inputs as mi

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
GUARD = 64
ZS = F32(1.1774100225154747)  # kNormalScale<true> = sqrt(2 ln 2), as normals_kernel rounds it to f32
_TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def _launch(fn: str, x: np.ndarray, n: int, out_dtype: type, out_width: int) -> np.ndarray:
    xd = torch.from_numpy(x.view(np.uint8)).to(DEV)
    out = poisoned((n * out_width + GUARD,), _TORCH[out_dtype], DEV)
    _lib.check(_lib.lib().smc_test_math_eval(_lib.TEST_MATH[fn], _lib.ptr(xd), n, _lib.ptr(out), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[n * out_width:]).all(), f"{fn}: wrote past element {n}"
    return got[:n * out_width]


def math_eval(fn: str, x: np.ndarray, out_dtype: type, in_width: int = 1, out_width: int = 1,
              head: np.ndarray | None = None) -> np.ndarray:
    """out[i] = fn(x[i]) on the device; x is [n] or [n, in_width].  The last workgroup of every launch is ragged:
    an n that is a multiple of 256 goes as two launches cut at n / 2 + 37.  head: HW_INCREMENT's coefficients."""
    x = np.ascontiguousarray(x)
    n = x.size // in_width
    assert x.size == n * in_width and 0 < n <= 1 << 24
    flat = x.reshape(n, in_width)
    cuts = [0, n] if n % 256 else [0, n // 2 + 37, n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        assert (hi - lo) % 256 != 0
        piece = np.ascontiguousarray(flat[lo:hi]).ravel()
        if head is not None:
            piece = np.concatenate([head.view(piece.dtype), piece])
        parts.append(_launch(fn, piece, hi - lo, out_dtype, out_width))
    out = np.concatenate(parts)
    return out.reshape(n, out_width) if out_width > 1 else out


def _pairs(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32))
    return np.stack([a, b], axis=1)


M = np.arange(1 << 23, dtype=np.uint32)
WORDS23 = (M << np.uint32(9)) | (M & np.uint32(0x1FF))  # every 23-bit field, the ignored low 9 bits varying


# ---- portable f32: device == oracle, bit for bit --------------------------------------------------------------------
def test_log_pos_bit_exact_over_every_uniform(oracle) -> None:
    u1 = mi.u1_all()
    assert_rows_equal(math_eval("LOG_POS", u1, F32), oracle.log_pos_n(u1), "LOG_POS")


@pytest.mark.parametrize("e", mi.Q_EXPONENTS)
def test_log_pos_bit_exact_over_the_greeks_domain(oracle, e) -> None:
    """q = x_T / X0 on both sides of 1 (greeks_log): every f32 in [2^-8, 2^8), one exponent per case."""
    q = mi.q_of_exponent(e)
    assert_rows_equal(math_eval("LOG_POS", q, F32), oracle.log_pos_n(q), "LOG_POS")


def test_sincos2pi_u24_bit_exact_over_every_angle(oracle) -> None:
    j = np.arange(1 << 24, dtype=np.uint32)
    assert_rows_equal(math_eval("SINCOS_U24", j, F32, out_width=2), oracle.sincos2pi_u24_n(j), "SINCOS_U24")


@pytest.mark.parametrize("fn", ["EXP2_ANY", "EXP_ANY"])
def test_exp_bit_exact_on_grid_and_edges(oracle, fn) -> None:
    """The CPU test's grid, ties, subnormal results and out-of-range edges (1e10 and +inf: inf; -inf and NaN: NaN on
    both sides)."""
    y = np.concatenate([mi.exp2_grid(), mi.exp2_ties(), mi.exp2_subnormal(), mi.EXP2_EDGES])
    got = math_eval(fn, y, F32)
    want = oracle.exp2_n(y) if fn == "EXP2_ANY" else oracle.exp_n(y)
    assert_rows_equal(got.view(np.uint32), want.view(np.uint32), fn)  # as bits: NaN and the sign of zero too
    if fn == "EXP2_ANY":
        tail = got[-mi.EXP2_EDGES.size:]

        def at(y: float) -> float:
            return float(tail[np.flatnonzero(mi.EXP2_EDGES == F32(y))[0]])

        assert at(1e10) == np.inf and at(3e38) == np.inf and at(128.0) == np.inf
        assert at(-1e10) == 0.0 and at(-3e38) == 0.0 and at(-151.0) == 0.0
        assert np.isnan(got[-1])
        # +inf: n stops at 128 and f = +inf; -inf: f = inf - inf (tests/test_math_accuracy.py says the same of the oracle)
        assert at(np.inf) == np.inf and np.isnan(at(-np.inf))


@pytest.mark.parametrize("b", [0, 1 << 31, 0xFFFFFFFF])
def test_normal_f32_bit_exact_over_every_radius(oracle, b) -> None:
    ab = _pairs(WORDS23, b)
    assert_rows_equal(math_eval("NORMAL_F32", ab, F32, 2, 2), oracle.normal_f32_n(ab[:, 0], ab[:, 1]), "NORMAL_F32")


@pytest.mark.parametrize("u1", [2.0**-23, 1.0, 0.5])
def test_normal_f32_bit_exact_over_every_angle(oracle, u1) -> None:
    ab = _pairs(mi.a_of_u1(u1) | 0x155, WORDS23)
    got = math_eval("NORMAL_F32", ab, F32, 2, 2)
    assert_rows_equal(got, oracle.normal_f32_n(ab[:, 0], ab[:, 1]), "NORMAL_F32")
    assert not np.isnan(got).any()
    if u1 == 1.0:  # radius sqrtf(-2 * +0) = -0: zeros of either sign, never NaN
        assert np.all(got == 0.0)


# ---- f64: device == oracle, bit for bit ------------------------------------------------------------------------------
def _bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(x).view(np.uint64)


def test_m2log_u32_bit_exact(oracle) -> None:
    a = np.concatenate([mi.m2log_structured(), mi.random_words(0)])
    assert_rows_equal(_bits(math_eval("M2LOG_U32", a, np.float64)), _bits(oracle.m2log_u32_n(a)), "M2LOG_U32")


def test_sincos2pi_u32_bit_exact(oracle) -> None:
    b = np.concatenate([mi.sincos_u32_structured(), mi.random_words(1)])
    assert_rows_equal(_bits(math_eval("SINCOS_U32", b, np.float64, out_width=2)), _bits(oracle.sincos2pi_u32_n(b)),
                      "SINCOS_U32")


def test_exp2s_bit_exact(oracle) -> None:
    ys = np.concatenate([mi.exp2s_structured(), mi.random_ys()])
    assert_rows_equal(_bits(math_eval("EXP2S", ys, np.float64)), _bits(oracle.exp2s_f64_n(ys)), "EXP2S")


def test_mul_exp2s_bit_exact(oracle) -> None:
    ys = mi.random_ys()
    x = np.random.default_rng([2024, 10]).uniform(1e-3, 1e3, ys.size)
    xy = np.concatenate([mi.mul_exp2s_structured(), np.stack([x, ys], axis=1)])
    assert_rows_equal(_bits(math_eval("MUL_EXP2S", xy, np.float64, in_width=2)), _bits(oracle.mul_exp2s_f64_n(xy)),
                      "MUL_EXP2S")


def test_normal_f64_bit_exact(oracle) -> None:
    sa, sb = mi.m2log_structured(), mi.sincos_u32_structured()
    a = np.concatenate([sa, mi.random_words(2, sb.size), mi.random_words(3)])
    b = np.concatenate([mi.random_words(4, sa.size), sb, mi.random_words(5)])
    ab = _pairs(a, b)
    assert_rows_equal(_bits(math_eval("NORMAL_F64", ab, np.float64, 2, 2)), _bits(oracle.normal_f64_n(a, b)),
                      "NORMAL_F64")


def test_twiddle_bit_exact(oracle) -> None:
    jn = mi.twiddle_pairs()
    assert_rows_equal(_bits(math_eval("TWIDDLE", jn, np.float64, 2, 2)), _bits(oracle.twiddle_n(jn)), "TWIDDLE")


def test_sqrt_radius_is_correctly_rounded(oracle) -> None:
    """sqrt_radius (rsq seed, Goldschmidt and Newton steps) equals the IEEE root (numpy's sqrt) on every radius
    squared of the structured and random words, the ends of its range, and the doubles beside 2^16 squares g^2,
    where the root lies next to a rounding boundary."""
    x = oracle.m2log_u32_n(np.concatenate([mi.m2log_structured(), mi.random_words(0)]))
    g = np.random.default_rng([2024, 11]).uniform(np.sqrt(2.3e-10), np.sqrt(46.1), 1 << 16)
    sq = g * g
    near = np.clip(np.concatenate([np.nextafter(sq, 0.0), sq, np.nextafter(sq, np.inf)]), 2.3e-10, 46.1)
    x = np.concatenate([x, [2.3e-10, 46.1], near])
    assert x.min() >= 2.3e-10 and x.max() <= 46.1
    assert_rows_equal(_bits(math_eval("SQRT_RADIUS", x, np.float64)), _bits(np.sqrt(x)), "SQRT_RADIUS")


# ---- SMC_MATH_HW: hardware transcendentals against f64 references of the exact inputs ------------------------------------
# The measured maxima HW_*_MAX_* and the asserted bounds HW_*_BOUND (twice each) are named in
# tests/helpers/math_inputs.py.
NORMAL_TOL = 2e-5  # the project's bound on an SMC_MATH_HW normal (test_hw_math_mode_within_fp32_tolerance)
MAX_RADIUS = 5.6468  # >= sqrt(46 ln 2), the radius at u1 = 2^-23

A_HALF = mi.a_of_u1(0.5)
ANGLE_WORDS = {"0": 0, "1/4": 1 << 30, "1/2": 1 << 31, "3/4": 3 << 30, "generic": 0x9E3779B9}
# the largest uniform below 1 is 1 - 2^-23 (u1 lies on the 2^-23 grid; 1 - 2^-24 is not drawn)
U1_SWEEPS = [2.0**-23, 0.5, 1.0 - 2.0**-23, 1.0]


def _u1_of(a: np.ndarray) -> np.ndarray:
    return 2.0 - (1.0 + (np.asarray(a, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) * 2.0**-23)


@functools.lru_cache(maxsize=None)
def _ref_tables() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """f64 references of the exact inputs, computed once: sqrt(-2 ln u1) by m = a >> 9, (cos, sin)(2 pi k 2^-23) by
    k = b >> 9 (libm in f64: errors of 1e-15 against bounds of 1e-7 and more)."""
    k = np.arange(1 << 23, dtype=np.float64)
    ang = 2.0 * np.pi * (k * 2.0**-23)
    return np.sqrt(-2.0 * np.log(_u1_of(WORDS23))), np.cos(ang), np.sin(ang)


def _normal_ref(ab: np.ndarray) -> np.ndarray:
    r, c, s = _ref_tables()
    m, k = ab[:, 0] >> np.uint32(9), ab[:, 1] >> np.uint32(9)
    return np.stack([r[m] * c[k], r[m] * s[k]], axis=1)


def _hw_sweeps() -> list:
    out = [pytest.param(WORDS23, w, id=f"angle {k}") for k, w in ANGLE_WORDS.items()]
    out += [pytest.param(mi.a_of_u1(u), WORDS23, id=f"u1 {u!r}") for u in U1_SWEEPS]
    return out


@pytest.fixture(scope="module")
def hw_factors() -> dict[str, np.ndarray]:
    """The two factors of the HW Box-Muller as the hot path's arithmetic returns them, HW_INCREMENT with coefficients
    (cb, ca) = (1, 0): ylo = fma(r * 1, cos, 0).  radius[m]: the sweep of u1 at angle 0, r cos(0) (cos(0) is exactly 1
    on this hardware: checked below at u1 = 1/2, where r = sqrt(-log2(1/2)) is exactly 1 too); cos / sin[k]: the sweep
    of the angle at u1 = 1/2."""
    head = np.array([1.0, 0.0], dtype=F32)
    radius = math_eval("HW_INCREMENT", _pairs(WORDS23, 0), F32, 2, 2, head=head)[:, 0]
    cs = math_eval("HW_INCREMENT", _pairs(A_HALF, WORDS23), F32, 2, 2, head=head)
    return {"radius": radius, "cos": cs[:, 0], "sin": cs[:, 1]}


def test_hw_factor_maxima(hw_factors) -> None:
    u1 = _u1_of(WORDS23)
    r, c, s = _ref_tables()
    dr = np.abs(hw_factors["radius"].astype(np.float64) * float(ZS) - r)
    ds = np.abs(hw_factors["sin"] - s)
    dc = np.abs(hw_factors["cos"] - c)
    print(f"HW radius max abs {dr.max():.4e} at u1 {u1[dr.argmax()]!r}; sin max abs {ds.max():.4e} at k {ds.argmax()}; "
          f"cos max abs {dc.max():.4e} at k {dc.argmax()}")
    print(f"HW at u1 = 1/2, angle 0: r cos {hw_factors['cos'][0]!r}, r sin {hw_factors['sin'][0]!r}; "
          f"u1 = 1: r {hw_factors['radius'][0]!r}")
    assert not np.isnan(hw_factors["radius"]).any() and not np.isnan(hw_factors["cos"]).any()
    # the fixture's identification: r is exact at u1 = 2^-1, 2^-4, 2^-16 (roots 1, 2, 4) and cos(0) = 1
    assert hw_factors["cos"][0] == 1.0 and hw_factors["sin"][0] == 0.0
    assert [float(hw_factors["radius"][mi.a_of_u1(2.0**-e) >> 9]) for e in (1, 4, 16)] == [1.0, 2.0, 4.0]
    assert hw_factors["radius"][0] == 0.0  # u1 = 1: sqrt(-0)
    assert dr.max() <= mi.HW_RADIUS_BOUND
    assert ds.max() <= mi.HW_SIN_BOUND
    assert dc.max() <= mi.HW_COS_BOUND
    # the per-factor constants compose to the project's bound on a normal: |dz| <= |dr| |trig| + r |dtrig|
    assert mi.HW_RADIUS_MAX_ABS + MAX_RADIUS * max(mi.HW_SIN_MAX_ABS, mi.HW_COS_MAX_ABS) < NORMAL_TOL


@pytest.mark.parametrize("a,b", _hw_sweeps())
def test_normal_f32_hw_over_each_factor(a, b) -> None:
    """NORMAL_F32_HW (normal_pair<true> as normals_kernel scales it) within 2e-5 of the f64 Box-Muller of its exact
    inputs over every radius at five angles and every angle at four radii; no NaN; zeros at u1 = 1.

    It also equals kNormalScale times HW_INCREMENT at (cb, ca) = (1, 0), bit for bit: both are r * trig of the shared
    helpers hw_radius / hw_cossin (the fma with a zero addend and a unit multiplier rounds once, as the product
    does), so hw_log_pair, the hot path's copy, is pinned to the normals' copy on every input swept here."""
    ab = _pairs(a, b)
    z = math_eval("NORMAL_F32_HW", ab, F32, 2, 2)
    err = np.abs(z - _normal_ref(ab))
    print(f"NORMAL_F32_HW max |z - z_ref| {err.max():.4e}")
    assert not np.isnan(z).any()
    assert err.max() <= NORMAL_TOL
    if np.ndim(a) == 0 and _u1_of(a) == 1.0:
        assert np.all(z == 0.0)
    y = math_eval("HW_INCREMENT", ab, F32, 2, 2, head=np.array([1.0, 0.0], dtype=F32))
    assert_rows_equal(z, ZS * y, "NORMAL_F32_HW vs HW_INCREMENT(1, 0)")


@pytest.mark.parametrize("a,b", _hw_sweeps())
def test_hw_increment_over_each_factor(hw_factors, a, b) -> None:
    """HW_INCREMENT (hw_log_pair: the per-pair arithmetic of hw_log_tail4, and per element of hw_log_increments4) at
    generic coefficients equals fmaf(cb r, trig, ca) built in numpy f32 from the factors, within 2 f32 ulp of the
    result's magnitude plus 2e-5 |cb|.  The numpy fma is an f64 product (exact) and sum rounded to f32, so it can
    differ from the device's single rounding in the last bit (measured: equal in every value of these sweeps); the
    bit-for-bit statement is test_normal_f32_hw_over_each_factor's."""
    cb, ca = F32(0.37), F32(-0.0123)
    ab = _pairs(a, b)
    y = math_eval("HW_INCREMENT", ab, F32, 2, 2, head=np.array([cb, ca], dtype=F32))
    m, k = ab[:, 0] >> np.uint32(9), ab[:, 1] >> np.uint32(9)
    br = (hw_factors["radius"][m] * cb).astype(np.float64)
    want = np.stack([(br * hw_factors["cos"][k] + float(ca)).astype(F32),
                     (br * hw_factors["sin"][k] + float(ca)).astype(F32)], axis=1)
    assert not np.isnan(y).any()
    tol = 2 * np.spacing(np.abs(want)).astype(np.float64) + NORMAL_TOL * float(abs(cb))
    err = np.abs(y.astype(np.float64) - want)
    print(f"HW_INCREMENT max |y - fma| {err.max():.4e}, exact in {float((y == want).mean()):.6f} of the values")
    assert np.all(err <= tol)


def test_hw_exp2_and_log_maxima() -> None:
    y = mi.exp2_grid()
    e = math_eval("HW_EXP2", y, F32).astype(np.float64)
    want = np.exp2(y.astype(np.float64))
    rel = np.abs(e - want) / want
    print(f"HW_EXP2 max rel {rel.max():.4e} at y {y[rel.argmax()]!r}")
    u1 = mi.u1_all()
    lg = math_eval("HW_LOG", u1, F32).astype(np.float64)
    wl = np.log(u1.astype(np.float64))
    low = u1 <= 0.5
    lrel = np.abs(lg[low] - wl[low]) / np.abs(wl[low])
    labs = np.abs(lg[~low] - wl[~low])
    print(f"HW_LOG max rel (u1 <= 1/2) {lrel.max():.4e}; max abs (u1 > 1/2) {labs.max():.4e}")
    assert not np.isnan(e).any() and not np.isnan(lg).any()
    assert lg[0] == 0.0  # ln 1
    assert rel.max() <= mi.HW_EXP2_BOUND
    assert lrel.max() <= mi.HW_LOG_REL_BOUND
    assert labs.max() <= mi.HW_LOG_ABS_BOUND


@pytest.mark.parametrize("e", mi.Q_EXPONENTS)
def test_hw_log_over_the_greeks_domain(e) -> None:
    """hw_log where greeks_log<.., true> takes it: every f32 q in [2^e, 2^(e + 1)) against numpy's f64 log, relative
    outside [1 / sqrt 2, sqrt 2) and absolute inside; twice the maxima measured over all 16 exponents."""
    q = mi.q_of_exponent(e)
    lg = math_eval("HW_LOG", q, F32)
    rel, ab = mi.log_q_errors(q, lg)
    print(f"HW_LOG on [2^{e}, 2^{e + 1}): max relative {rel:.4e}, max absolute {ab:.4e}")
    assert not np.isnan(lg).any()
    if e == 0:
        assert lg[0] == 0.0
    assert rel <= mi.HW_LOG_Q_REL_BOUND
    assert ab <= mi.HW_LOG_Q_ABS_BOUND
