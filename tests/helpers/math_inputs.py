"""Input sets of the device-math tests, shared by the CPU tests of the oracle's restatement
(tests/test_math_accuracy.py) and the GPU tests of the device functions (tests/test_gpu_math.py), so both sides
are pinned at the same points, and the accuracy bounds both assert, each named once.  Pure numpy; no GPU, no oracle."""

from __future__ import annotations

import numpy as np

# ---- accuracy bounds ---------------------------------------------------------------------------------------------
# The maximum errors the sweeps assert, each named once: test_math_accuracy.py (portable, on the CPU restatement) and
# test_gpu_math.py (SMC_MATH_HW, on the device) assert against these names, and tests/helpers/basket_reference.py
# builds its a-priori bounds from them, so a bound and the sweep that justifies it cannot drift apart.
# Portable f32 (fixed IEEE sequences; the measured maxima rounded up in the last digit shown):
LOG_POS_MAX_REL = 1.67e-7  # log_pos over all 2^23 u1
LOG_POS_MAX_ABS = 5.4e-7
RADIUS_MAX_ABS = 3.5e-7  # |sqrtf(-2 log_pos(u1)) - sqrt(-2 ln u1)| over all 2^23 u1
SINCOS_MAX_ABS = 8.6e-8  # sincos2pi_u24 over all 2^24 angles
EXP2_MAX_REL = 7.7e-8  # exp2_any on the 2^-16 grid over [-126, 127]
# log_pos over q_all(): every f32 in [2^-8, 2^8), the domain greeks_log takes it on (measured 1.2717e-7 and 4.8878e-8)
LOG_POS_Q_MAX_REL = 1.28e-7  # relative, q outside [1 / sqrt 2, sqrt 2)
LOG_POS_Q_MAX_ABS = 4.9e-8  # absolute, q inside it
# SMC_MATH_HW: maxima measured on an MI355X over the whole domain of each factor (the hardware is deterministic per
# input, so these are the true maxima of this build); the tests assert twice each (the *_BOUND names), which leaves
# room for a compiler that lowers a builtin through another instruction form and nothing else.
HW_RADIUS_MAX_ABS = 3.9460e-07  # |kNormalScale r - sqrt(-2 ln u1)| over all 2^23 u1
HW_SIN_MAX_ABS = 1.2527e-07  # over all 2^23 angles
HW_COS_MAX_ABS = 1.2527e-07
HW_EXP2_MAX_REL = 8.1403e-08  # v_exp_f32 on the 2^-16 grid over [-126, 127]
HW_LOG_MAX_REL = 1.6095e-07  # hw_log over the u1 <= 1/2
HW_LOG_MAX_ABS = 7.2019e-08  # hw_log over the u1 > 1/2 (ln u1 -> 0)
HW_LOG_Q_MAX_REL = 1.6326e-07  # hw_log over q_all() outside [1 / sqrt 2, sqrt 2) (at q in [2^-5, 2^-4))
HW_LOG_Q_MAX_ABS = 3.2230e-08  # hw_log over q_all() inside it (at q in [1 / sqrt 2, 1))
HW_RADIUS_BOUND = 2 * HW_RADIUS_MAX_ABS
HW_SIN_BOUND = 2 * HW_SIN_MAX_ABS
HW_COS_BOUND = 2 * HW_COS_MAX_ABS
HW_EXP2_BOUND = 2 * HW_EXP2_MAX_REL
HW_LOG_REL_BOUND = 2 * HW_LOG_MAX_REL
HW_LOG_ABS_BOUND = 2 * HW_LOG_MAX_ABS
HW_LOG_Q_REL_BOUND = 2 * HW_LOG_Q_MAX_REL
HW_LOG_Q_ABS_BOUND = 2 * HW_LOG_Q_MAX_ABS

# ---- portable f32 ------------------------------------------------------------------------------------------------


def u1_all() -> np.ndarray:
    """The 2^23 values u1 = 2 - 1.m the f32 Box-Muller can draw (smc_rng.h): (0, 1] on the 2^-23 grid, in the
    order of m = a >> 9 (m = 0 gives 1.0, m = 2^23 - 1 gives 2^-23)."""
    m = np.arange(1 << 23, dtype=np.uint32)
    return (np.float32(2.0) - (m | np.uint32(0x3F800000)).view(np.float32)).astype(np.float32)


def a_of_u1(u1: float) -> int:
    """A stream word a (low 9 bits zero) whose f32 uniform is u1 = 2 - 1.m(a >> 9)."""
    m = int(round((2.0 - u1) * 2.0**23)) - (1 << 23)
    assert 0 <= m < 1 << 23 and 2.0 - (1.0 + m * 2.0**-23) == u1
    return m << 9


Q_EXPONENTS = tuple(range(-8, 8))


def q_of_exponent(e: int) -> np.ndarray:
    """The 2^23 f32 values in [2^e, 2^(e + 1)): every mantissa at one binary exponent."""
    assert -126 <= e <= 127
    return (np.uint32((e + 127) << 23) | np.arange(1 << 23, dtype=np.uint32)).view(np.float32)


def q_all():
    """The domain greeks_log takes the logs on, q = x_T / X0 in [2^-8, 2^8) (v sqrt(T) up to about 1.1 at five standard
    deviations): every f32 in it, one exponent at a time."""
    return (q_of_exponent(e) for e in Q_EXPONENTS)


def log_q_errors(q: np.ndarray, got: np.ndarray) -> tuple[float, float]:
    """(max relative error of got against numpy's f64 log over the q outside [1 / sqrt 2, sqrt 2), max absolute error
    over those inside it); 0 where a side is empty."""
    q64 = q.astype(np.float64)
    want = np.log(q64)
    err = np.abs(got.astype(np.float64) - want)
    inside = (q64 >= np.sqrt(0.5)) & (q64 < np.sqrt(2.0))
    rel = float((err[~inside] / np.abs(want[~inside])).max()) if not inside.all() else 0.0
    return rel, float(err[inside].max()) if inside.any() else 0.0


EXP2_EDGES = np.array(
    [-1e10, -3e38, -151.0, -150.5, -150.0, -149.5, -149.0, -148.5, -127.5, -126.5, -126.0, -125.5, -0.0, 0.0, 126.5,
     127.0, 127.5, 127.99999, 128.0, 128.5, 129.0, 1e10, 3e38, np.inf, -np.inf, np.nan], dtype=np.float32)


def exp2_grid() -> np.ndarray:
    """i 2^-16 for i in [-126 2^16, 127 2^16]: every f32 on that grid over the normal range of 2^y."""
    i = np.arange(-126 << 16, (127 << 16) + 1, dtype=np.int64)
    return (i.astype(np.float64) * 2.0**-16).astype(np.float32)  # exact: 23 significant bits at most


def exp2_ties() -> np.ndarray:
    """k + 1/2 for every integer k in [-150, 127]: rintf rounds to even, so f alternates between -1/2 and +1/2."""
    return (np.arange(-150, 128, dtype=np.float64) + 0.5).astype(np.float32)


def exp2_subnormal() -> np.ndarray:
    """y in [-149, -126) on a 2^-8 grid: subnormal results (ldexpf rounds the polynomial's value once)."""
    return (np.arange(-149 * 256, -126 * 256, dtype=np.float64) / 256.0).astype(np.float32)


# ---- f64: structured sets ----------------------------------------------------------------------------------------


def m2log_table_index(a: np.ndarray) -> np.ndarray:
    """Table row i of m2log_u32(a) (smc_math.h): (mh + 2^9) >> 10 of the top 20 mantissa bits of a + 1/2."""
    m = np.asarray(a, dtype=np.uint32).astype(np.float64) + 0.5
    mh = (m.view(np.uint64) >> np.uint64(32)).astype(np.int64) & 0xFFFFF
    return (mh + 0x200) >> 10


def m2log_structured() -> np.ndarray:
    """The edges of m2log_u32's input domain: the ends, every exponent change (2^k - 1, 2^k), the words on either
    side of each of the 1024 rounding boundaries of the table index (rows 0|1 .. 1023|1024) at the exponents
    e = 32 (a in [2^31, 2^32): mh = (2 a + 1 - 2^32) >> 12) and e = 20 (a in [2^19, 2^20): mh = 2 a + 1 - 2^20, odd),
    and the word nearest 2^32 / sqrt(2)."""
    words = [0, 1, 2, 3, 0xFFFFFFFE, 0xFFFFFFFF, 0xB504F333]
    for k in range(1, 33):
        words += [2**k - 1] + ([2**k] if k < 32 else [])
    i = np.arange(1, 1025, dtype=np.int64)
    hi32 = (1 << 31) + ((1024 * i - 512) << 11)       # first word of row i at e = 32
    lo20 = (1 << 19) + 512 * i - 257                  # last word of row i - 1 at e = 20
    out = np.concatenate([np.array(words, dtype=np.int64), hi32 - 1, hi32, lo20, lo20 + 1])
    assert out.min() >= 0 and out.max() < 1 << 32
    return out.astype(np.uint32)


SINCOS_U32_EDGES = np.array([0, 1, 2**29 - 1, 2**29, 2**30, 3 * 2**29, 2**31, 2**32 - 2**29, 2**32 - 1], dtype=np.uint32)


def sincos_u32_structured() -> np.ndarray:
    """Every table index b & 1023 at the offsets b >> 10 (signed 22 bits) in {0, 1, 2^21 - 1, -2^21, -1}, and the
    quarter-turn edges."""
    j = np.arange(1024, dtype=np.int64)
    parts = [SINCOS_U32_EDGES.astype(np.int64)]
    for y in (0, 1, 2**21 - 1, -(2**21), -1):
        parts.append(((y & 0x3FFFFF) << 10) | j)
    return np.concatenate(parts).astype(np.uint32)


EXP2S_EDGES = np.array([-258000.0, -18000.5, -0.5, -1e-300, 0.0, 1e-12, 0.5, 127.49, 128.0, 18000.0, 258000.0])


def exp2s_structured() -> np.ndarray:
    """ys of exp2s_f64: the edge list, the ties n +- 1/2 (the magic-number rounding is to even) for 513 integers n,
    which also take every table index n mod 256 and both signs of the exponent n >> 8, and the same n exactly and a
    quarter off."""
    n = np.arange(-256, 257, dtype=np.float64)
    return np.concatenate([EXP2S_EDGES, n - 0.5, n + 0.5, n, n + 0.25])


def mul_exp2s_structured() -> np.ndarray:
    """[n, 2] rows (x, ys): exp2s_structured() at x in {1, 100, 1e-3}."""
    ys = exp2s_structured()
    return np.concatenate([np.stack([np.full_like(ys, x), ys], axis=1) for x in (1.0, 100.0, 1e-3)])


# ---- f64: bulk random points (one seed, so the CPU and GPU tests see the same) -------------------------------------
N_RANDOM = 1 << 22


def random_words(stream: int, n: int = N_RANDOM) -> np.ndarray:
    return np.random.default_rng([2024, stream]).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def random_ys(n: int = N_RANDOM) -> np.ndarray:
    """Path exponents in units of ln 2 / 256 over +-22000 (e^+-60, the range of the existing test)."""
    return np.random.default_rng([2024, 9]).uniform(-22000.0, 22000.0, n)


TWIDDLE_SIZES = (4, 12, 1000, 1024, 2048)


def twiddle_pairs() -> np.ndarray:
    """[n, 2] int64 rows (j, N): every j < N of each DFT size."""
    return np.concatenate([np.stack([np.arange(N, dtype=np.int64), np.full(N, N, dtype=np.int64)], axis=1)
                           for N in TWIDDLE_SIZES])


# ---- references ----------------------------------------------------------------------------------------------------


def sincos_u32_angle_units(b: np.ndarray) -> np.ndarray:
    """The angle of the f64 Box-Muller word b in units of 2^-32 turn, as an integer in [0, 2^32):
    (b mod 1024) 2^22 + (b >> 10 as a signed 22-bit integer)."""
    b = np.asarray(b, dtype=np.uint32).astype(np.int64)
    y = (b >> 10) - np.where(b >= 1 << 31, 1 << 22, 0)
    return ((b & 1023) * (1 << 22) + y) % (1 << 32)


def sincos_turns_longdouble(units: np.ndarray, bits: int) -> tuple[np.ndarray, np.ndarray]:
    """(sin, cos)(2 pi units 2^-bits) in long double after an exact integer reduction to the nearest quarter
    turn (x87 long double: 64-bit significand; at least as precise as double elsewhere)."""
    units = np.asarray(units, dtype=np.int64)
    quarter = 1 << (bits - 2)
    k = (units + quarter // 2) // quarter
    x = np.longdouble("6.283185307179586476925286766559005768") * (units - k * quarter).astype(np.longdouble) \
        / np.longdouble(2**bits)
    s, c = np.sin(x), np.cos(x)
    q = k % 4
    sin = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    cos = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    return sin, cos
