"""How accurate the device math functions are (csrc/smc_math.h, restated op for op by oracle/gbm_oracle.c), swept
over their whole input domains on the CPU restatement; tests/test_gpu_math.py shows the device functions equal
the restatement bit for bit over the same inputs.  CPU only.

The portable f32 functions are fixed sequences of IEEE operations, so their maximum errors are constants of the
code: the bounds below are the maxima measured against libm in f64 (log_pos: relative 1.661e-7, absolute 5.33e-7;
radius 3.47e-7; sin / cos 8.516e-8; exp2 7.647e-8), rounded up in the last digit shown.  A coefficient change has to
move them deliberately (each is named once, in tests/helpers/math_inputs.py).  The f64 functions keep the bounds of
test_oracle.py's sampled test (2 ulp; 2^-52 absolute for sin / cos), now at the structured points of tests/helpers/math_inputs.py against mpmath (60 digits) and at 2^22
random points against numpy long double (an f64 libm reference of x 2^(ys/256) carries up to 1.5 ulp of its own)."""

from __future__ import annotations

import numpy as np
import pytest

from tests.helpers import math_inputs as mi

F32 = np.float32


# ---- portable f32 ------------------------------------------------------------------------------------------------
def test_log_pos_over_every_uniform(oracle) -> None:
    u1 = mi.u1_all()
    assert u1.size == 1 << 23 and u1[0] == 1.0 and u1[-1] == F32(2.0**-23) and np.all(np.diff(u1) < 0)
    got = oracle.log_pos_n(u1)
    want = np.log(u1.astype(np.float64))
    err = np.abs(got.astype(np.float64) - want)
    nz = want != 0.0
    rel, ab = float((err[nz] / np.abs(want[nz])).max()), float(err.max())
    print(f"log_pos: max relative {rel:.4e}, max absolute {ab:.4e}")
    assert rel <= mi.LOG_POS_MAX_REL
    assert ab <= mi.LOG_POS_MAX_ABS
    # the Box-Muller radius as box_muller<false> forms it: sqrtf(-2 log_pos(u1))
    radius = np.sqrt(F32(-2.0) * got)
    assert radius.dtype == np.float32
    rerr = float(np.abs(radius.astype(np.float64) - np.sqrt(-2.0 * want)).max())
    print(f"radius: max absolute {rerr:.4e}")
    assert rerr <= mi.RADIUS_MAX_ABS
    assert got[0] == 0.0 and not np.signbit(got[0])  # log_pos(1.0f) == +0.0f exactly
    assert np.all(got[1:] < 0.0)


@pytest.mark.parametrize("e", mi.Q_EXPONENTS)
def test_log_pos_over_the_greeks_domain(oracle, e) -> None:
    """log_pos where greeks_log takes it: q = x_T / X0 on both sides of 1, every mantissa of one binary exponent per
    case, against numpy's f64 log.  Relative outside [1 / sqrt 2, sqrt 2), absolute inside (what hv and hT feel)."""
    q = mi.q_of_exponent(e)
    assert q.size == 1 << 23 and q[0] == F32(2.0**e) and np.all(np.diff(q) > 0) and q[-1] < F32(2.0 ** (e + 1))
    got = oracle.log_pos_n(q)
    rel, ab = mi.log_q_errors(q, got)
    print(f"log_pos on [2^{e}, 2^{e + 1}): max relative {rel:.4e}, max absolute {ab:.4e}")
    assert rel <= mi.LOG_POS_Q_MAX_REL
    assert ab <= mi.LOG_POS_Q_MAX_ABS
    assert np.all(np.diff(got) >= 0)  # monotone over the exponent
    if e == 0:
        assert got[0] == 0.0 and not np.signbit(got[0])


def test_sincos2pi_u24_over_every_angle(oracle) -> None:
    j = np.arange(1 << 24, dtype=np.uint32)
    sc = oracle.sincos2pi_u24_n(j)
    ang = 2.0 * np.pi * j.astype(np.float64) * 2.0**-24
    es = float(np.abs(sc[:, 0] - np.sin(ang)).max())
    ec = float(np.abs(sc[:, 1] - np.cos(ang)).max())
    print(f"sincos2pi_u24: max absolute sin {es:.4e}, cos {ec:.4e}")
    assert es <= mi.SINCOS_MAX_ABS and ec <= mi.SINCOS_MAX_ABS
    # the four quarter turns are exact (and j = 2^24, the k = 4 branch of the reduction, is the turn again)
    q = oracle.sincos2pi_u24_n(np.array([0, 1 << 22, 1 << 23, 3 << 22, 1 << 24], dtype=np.uint32))
    np.testing.assert_array_equal(q, np.array([[0, 1], [1, 0], [0, -1], [-1, 0], [0, 1]], dtype=np.float32))
    norm = sc[:, 0].astype(np.float64) ** 2 + sc[:, 1].astype(np.float64) ** 2
    assert float(np.abs(norm - 1.0).max()) <= 4 * 2.0**-24


def test_exp2_any_grid_and_edges(oracle) -> None:
    y = mi.exp2_grid()
    assert y.size == 253 * 65536 + 1 and y[0] == -126.0 and y[-1] == 127.0
    got = oracle.exp2_n(y).astype(np.float64)
    want = np.exp2(y.astype(np.float64))
    rel = float((np.abs(got - want) / want).max())
    print(f"exp2_any: max relative {rel:.4e}")
    assert rel <= mi.EXP2_MAX_REL
    # integers: exact powers of two over the whole finite range, subnormal results included
    k = np.arange(-149, 128)
    np.testing.assert_array_equal(oracle.exp2_n(k.astype(F32)), np.ldexp(F32(1.0), k).astype(F32))
    # ties k + 1/2: rintf rounds to even, f = +-1/2 alternately; both ends of the polynomial's interval
    t = mi.exp2_ties()
    normal = t >= -126
    tie = oracle.exp2_n(t).astype(np.float64)
    want_t = np.exp2(t.astype(np.float64))
    assert float((np.abs(tie - want_t) / want_t)[normal].max()) <= mi.EXP2_MAX_REL
    n = np.rint(t)
    assert set(np.unique(t - n)) == {-0.5, 0.5}
    # subnormal results: the polynomial's value rounded once by ldexpf, so within half a subnormal ulp (2^-150)
    # plus the polynomial's relative error
    ys = mi.exp2_subnormal()
    sub = oracle.exp2_n(ys).astype(np.float64)
    want_s = np.exp2(ys.astype(np.float64))
    assert np.all(np.abs(sub - want_s) <= 2.0**-150 + mi.EXP2_MAX_REL * want_s)
    assert np.all((sub > 0) & (sub < 2.0**-126))
    assert np.all(np.diff(sub) >= 0)
    # out of range, finite: 0 below -150, inf from 128 up; the float -> int conversion saturates as the device's does
    # (a bare C cast of 1e10f gave INT_MIN here and so 0)
    edges = {-1e10: 0.0, -3e38: 0.0, -151.0: 0.0, -150.5: 0.0, 128.0: np.inf, 128.5: np.inf, 129.0: np.inf,
             1e10: np.inf, 3e38: np.inf, -149.0: 2.0**-149, -0.0: 1.0, 0.0: 1.0}
    got_e = oracle.exp2_n(np.array(list(edges), dtype=F32))
    np.testing.assert_array_equal(got_e, np.array(list(edges.values()), dtype=F32))
    assert not np.signbit(got_e[:4]).any()
    assert np.isnan(oracle.exp2_n(np.array([np.nan], dtype=F32))[0])
    assert oracle.lib().oracle_exp2(1e10) == np.inf  # the scalar wrapper too
    # -150 and -149.5 round to n = -150 (ties to even) and n = -150 / -149: 2^-150 (1 + ...) rounds to 0 or 2^-149
    assert oracle.exp2_n(np.array([-150.0], dtype=F32))[0] == 0.0
    assert oracle.exp2_n(np.array([-149.5], dtype=F32))[0] == F32(2.0**-149)


def test_exp2_any_of_plus_infinity_is_infinity(oracle) -> None:
    """exp2_any(+inf) is +inf: n = rintf(fminf(y, 128)) stops at 128, so f = y - n is +inf (not inf - inf), the
    polynomial of positive coefficients is +inf and ldexpf keeps it.  fminf drops a NaN but f = NaN - 128 keeps it;
    -inf still splits into inf - inf and gives NaN.  tests/test_gpu_math.py holds the device to the same bits."""
    got = oracle.exp2_n(np.array([np.inf, np.nan, -np.inf], dtype=F32))
    assert got[0] == np.inf and np.isnan(got[1]) and np.isnan(got[2])
    # capping n changes no finite result: beside the cap the split is what rintf alone gives, above it all is inf
    y = np.array([127.49999, 127.5, 127.99999, 128.0, 128.00002, 128.5, 200.0, 2147483648.0, 3.4028235e38], dtype=F32)
    got = oracle.exp2_n(y)
    np.testing.assert_array_equal(got[3:], np.full(6, np.inf, dtype=F32))
    want = np.exp2(y[:3].astype(np.float64))
    assert np.all(np.abs(got[:3].astype(np.float64) - want) <= mi.EXP2_MAX_REL * want)


def test_exp_any_is_exp2_any_of_the_scaled_argument(oracle) -> None:
    x = np.concatenate([np.linspace(-87.0, 88.0, 200001), [1e10, -1e10, 3e38, -3e38]]).astype(F32)
    with np.errstate(over="ignore"):
        scaled = x * F32(1.44269502)  # 3e38 overflows to inf, as on the device
    np.testing.assert_array_equal(oracle.exp_n(x), oracle.exp2_n(scaled))
    assert np.isnan(oracle.exp_n(np.array([np.nan], dtype=F32))[0])


def test_normal_f32_array_form_matches_the_stream(oracle) -> None:
    """oracle_normal_f32_n / oracle_normal_f64_n are the Box-Muller the normals are drawn with: the first pairs of
    a stream, fed to them, give oracle.normals' values."""
    w = oracle.stream_u32(7, 3, 5, 8)  # T = 4: group 5's own stream, one pair per path and step pair
    z32 = oracle.normal_f32_n(w[0::2], w[1::2])
    z64 = oracle.normal_f64_n(w[0::2], w[1::2])
    n32 = oracle.normals(7, 3, 4, 24, "float32")[:2, 20:24]
    n64 = oracle.normals(7, 3, 4, 24, "float64")[:2, 20:24]
    np.testing.assert_array_equal(z32.T, n32)
    np.testing.assert_array_equal(z64.T, n64)


# ---- f64 -----------------------------------------------------------------------------------------------------------
def _ulps(got: np.ndarray, want_ld: np.ndarray) -> float:
    """max |got - want| in ulps of want (rounded to double)."""
    w64 = np.abs(want_ld.astype(np.float64))
    return float((np.abs(got.astype(np.longdouble) - want_ld) / np.spacing(w64)).max())


def test_structured_sets_reach_what_they_name() -> None:
    a = mi.m2log_structured()
    idx = mi.m2log_table_index(a[-4096:]).reshape(4, 1024)
    rows = np.arange(1024)
    np.testing.assert_array_equal(idx[0], rows)      # e = 32: last word of row i - 1 ...
    np.testing.assert_array_equal(idx[1], rows + 1)  # ... and first word of row i, i = 1..1024
    np.testing.assert_array_equal(idx[2], rows)      # e = 20
    np.testing.assert_array_equal(idx[3], rows + 1)
    e = np.frexp(a[-4096:].astype(np.float64) + 0.5)[1].reshape(4, 1024)
    assert np.all(e[:2] == 32) and np.all(e[2:] == 20)
    assert set(np.frexp(a.astype(np.float64) + 0.5)[1]) == set(range(33))  # every exponent 0..32
    b = mi.sincos_u32_structured()
    assert set(b & 1023) == set(range(1024))
    ys = mi.exp2s_structured()
    assert set(np.rint(ys).astype(np.int64) % 256) == set(range(256))


def test_f64_functions_at_structured_points_against_mpmath(oracle) -> None:
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    a = mi.m2log_structured()
    got = oracle.m2log_u32_n(a)
    for ai, g in zip(a.tolist(), got.tolist()):
        want = -2 * mp.log((mp.mpf(ai) + mp.mpf("0.5")) / 2**32)
        assert abs(mp.mpf(g) - want) <= 2 * mp.mpf(float(np.spacing(float(want)))), hex(ai)
    b = mi.sincos_u32_structured()
    sc = oracle.sincos2pi_u32_n(b)
    units = mi.sincos_u32_angle_units(b)
    for bi, ui, (s, c) in zip(b.tolist(), units.tolist(), sc.tolist()):
        x = 2 * mp.pi * ui / 2**32
        assert abs(mp.mpf(s) - mp.sin(x)) <= mp.mpf(2) ** -52 and abs(mp.mpf(c) - mp.cos(x)) <= mp.mpf(2) ** -52, hex(bi)
    xy = mi.mul_exp2s_structured()
    got_m = oracle.mul_exp2s_f64_n(xy)
    got_e = oracle.exp2s_f64_n(xy[:, 1])
    for (x, ys), gm, ge in zip(xy.tolist(), got_m.tolist(), got_e.tolist()):
        e = mp.power(2, mp.mpf(ys) / 256)
        assert abs(mp.mpf(ge) - e) <= 2 * mp.mpf(float(np.spacing(float(e)))), ys
        want = mp.mpf(x) * e
        assert abs(mp.mpf(gm) - want) <= 2 * mp.mpf(float(np.spacing(float(want)))), (x, ys)


def test_f64_functions_at_random_points(oracle) -> None:
    a = np.concatenate([mi.m2log_structured(), mi.random_words(0)])
    want = -2.0 * np.log((a.astype(np.longdouble) + np.longdouble(0.5)) / np.longdouble(2.0**32))
    u = _ulps(oracle.m2log_u32_n(a), want)
    print(f"m2log_u32: max {u:.3f} ulp")
    assert u <= 2.0
    b = np.concatenate([mi.sincos_u32_structured(), mi.random_words(1)])
    sc = oracle.sincos2pi_u32_n(b)
    s, c = mi.sincos_turns_longdouble(mi.sincos_u32_angle_units(b), 32)
    es, ec = float(np.abs(sc[:, 0] - s).max()), float(np.abs(sc[:, 1] - c).max())
    print(f"sincos2pi_u32: max absolute sin {es:.3e}, cos {ec:.3e}")
    assert es <= 2.0**-52 and ec <= 2.0**-52
    ys = np.concatenate([mi.exp2s_structured(), mi.random_ys()])
    e = np.exp2(ys.astype(np.longdouble) / 256)
    u = _ulps(oracle.exp2s_f64_n(ys), e)
    print(f"exp2s_f64: max {u:.3f} ulp")
    assert u <= 2.0
    for x in (1.0, 100.0, 1e-3):
        u = _ulps(oracle.mul_exp2s_f64_n(np.stack([np.full_like(ys, x), ys], axis=1)), np.longdouble(x) * e)
        print(f"mul_exp2s_f64(x = {x}): max {u:.3f} ulp")
        assert u <= 2.0


def test_twiddles_against_long_double(oracle) -> None:
    """twiddle (the N-point DFT's (sin, cos)(2 pi j / N)): within 2^-52 absolute, exact at the quarter turns."""
    jn = mi.twiddle_pairs()
    sc = oracle.twiddle_n(jn)
    j, N = jn[:, 0], jn[:, 1]
    k = (8 * j + N) // (2 * N)
    x = np.longdouble("6.283185307179586476925286766559005768") * (4 * j - k * N).astype(np.longdouble) / (4 * N)
    s, c = np.sin(x), np.cos(x)
    q = k % 4
    ws = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    wc = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    assert float(np.abs(sc[:, 0] - ws).max()) <= 2.0**-52 and float(np.abs(sc[:, 1] - wc).max()) <= 2.0**-52
    np.testing.assert_array_equal(oracle.twiddle_n(np.array([[0, 4], [1, 4], [2, 4], [3, 4]])),
                                  np.array([[0, 1], [1, 0], [0, -1], [-1, 0]], dtype=np.float64))
