"""The float64 reference of the basket Greeks (tests/helpers/basket_greeks_reference.py) held to what it claims, on the
CPU, and the float32 restatement of the header's table (tests/helpers/basket_greeks_restate.py: the CPU expectation of
basket_greeks_kernel in portable math) held to the reference.

1. The reference's Greeks against central differences of the reference's own Monte-Carlo price on the same words: the
   pathwise estimator is the derivative of that price, so the two agree to the error of the difference quotient.
2. A = 1 against the Black-Scholes closed forms, within the Monte-Carlo error.
3. The restatement on the oracle's kernel-mode terminal values against the reference, as a share of each column's
   standard error: the measurement behind the tolerance of tests/test_gpu_basket_greeks.py."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests.helpers import basket_greeks_cases as cases
from tests.helpers import basket_greeks_reference as gr
from tests.helpers import basket_greeks_restate as rs
from tests.helpers import basket_reference as br

SEED, ORD0 = cases.SEED, cases.ORD0
REL_STEP = 1e-5


def _finite_difference_shares(oracle, A: int, normalize: bool, dfactor=None) -> dict[str, float]:
    """The largest |central difference - pathwise Greek| / tolerance by kind of Greek, over 4 Sobol contracts, both
    payoffs and every asset.  T = 3 steps, P = 2048 paths.

    Step h: 1e-5 X0_i, 1e-5 T, and 1e-5 absolute for v_i, r and rho.  The tolerance, from the reference's own values:
    * truncation: the central difference at h errs by h^2 f''' / 6 and the one at 2 h by four times that, so their
      difference is three times the truncation error at h: |D(2h) - D(h)| is allowed;
    * cancellation: a path's payoff comes from T + 16 float64 operations at most (the cumulated exponent, exp, the
      scale, the basket, the payoff, the mean), the exponent's error growing with |ln(x / X0)|, so a price is off by at
      most eps_V df (K + mean bk) with eps_V = (T + 16) 2^-52 (1 + max |ln(x / X0)|), and the quotient by eps_V
      df (K + mean bk) / h;
    * kinks: a path whose basket lies within 1.5 h |d bk / d theta| of the strike changes its exercise inside the
      step; its share of the quotient and its pathwise term then differ by at most df |d bk / d theta| / P."""
    T, P, B = 3, 2048, 4
    rows = cases.sobol_rows(oracle, A, B)
    z, _ = gr.words_and_drivers(oracle, B, A, T, P, SEED, ORD0)
    if dfactor is not None:
        keep, gr.dfactor = gr.dfactor, dfactor
    try:
        r = gr.path_terms(rows, A, T, z, normalize)
    finally:
        if dfactor is not None:
            gr.dfactor = keep
    block = gr.block_of(r["t"], A)
    K, Tm, _, _, X0, _, _ = br.fields(rows, A)
    xT = gr._terminal(rows, A, T, z)
    eps_v = (T + 16) * 2.0 ** -52 * (1.0 + np.abs(np.log(xT / X0[:, :, None])).max(axis=(1, 2)))
    scale = r["df"] * (K + r["bk"].mean(axis=1))
    one = np.full(B, REL_STEP)
    # (kind, row field, put column, call column, step, sign of the reported Greek)
    params = [("delta", 4 + i, i, A + i, REL_STEP * X0[:, i], 1.0) for i in range(A)]
    params += [("vega", 4 + 2 * A + i, 2 * A + i, 3 * A + i, one, 1.0) for i in range(A)]
    params += [("rho", 2, 4 * A, 4 * A + 1, one, 1.0), ("theta", 1, 4 * A + 2, 4 * A + 3, REL_STEP * Tm, -1.0),
               ("correlation", 3, 4 * A + 4, 4 * A + 5, one, 1.0)]
    used: dict[str, float] = {}
    for index, (kind, field, put_col, call_col, h, sign) in enumerate(params):
        def quotient(step: np.ndarray) -> np.ndarray:
            up, down = rows.copy(), rows.copy()
            up[:, field] += step
            down[:, field] -= step
            return sign * (gr.prices(up, A, T, z, normalize) - gr.prices(down, A, T, z, normalize)) / (2 * step[:, None])

        d1, d2 = quotient(h), quotient(2 * h)
        slope = np.abs(r["dbk"][index])
        crossing = np.abs(K[:, None] - r["bk"]) <= 1.5 * h[:, None] * slope
        kink = (crossing * r["df"][:, None] * slope).sum(axis=1) / P
        tol = np.abs(d2 - d1) + (kink + eps_v * scale / h)[:, None]
        err = np.abs(d1 - block[:, [put_col, call_col]])
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0.0, 0.0, err / tol)
        used[kind] = max(used.get(kind, 0.0), float(np.where(np.isnan(share), np.inf, share).max()))
    return used


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 8])
def test_reference_greeks_are_the_derivatives_of_the_reference_price(oracle, A, normalize) -> None:
    used = _finite_difference_shares(oracle, A, normalize)
    print(f"A {A} {'NORMALIZE' if normalize else 'RAW'}: share of the tolerance used " +
          ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert set(used) == {"delta", "vega", "rho", "theta", "correlation"}
    assert max(used.values()) < 1.0, used


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A", [2, 4])
def test_a_wrong_factor_derivative_leaves_the_tolerance(oracle, A, normalize) -> None:
    """G = Phi(S) in the place of Lc Phi(S) Lc^-1 (dLc = Phi(S) Lc in the place of Lc Phi(S)) is off by a fifth in the
    correlation columns: the test above has to see it, and only there."""
    def wrong(n: int, rho: float) -> np.ndarray:
        Lc = br.factor(n, rho)
        Li = np.linalg.inv(Lc)
        S = Li @ (np.ones((n, n)) - np.eye(n)) @ Li.T
        return (np.tril(S, -1) + 0.5 * np.diag(np.diag(S))) @ Lc

    used = _finite_difference_shares(oracle, A, normalize, dfactor=wrong)
    print(f"A {A}: wrong factor derivative, share of the tolerance used {used}")
    assert used["correlation"] > 100.0, used
    assert max(v for k, v in used.items() if k != "correlation") < 1.0, used


def _ncdf(x: float) -> float:
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def _black_scholes(K: float, T: float, r: float, X0: float, d: float, v: float) -> list[float]:
    """delta, vega, rho, theta (-dV/dT per year) of the European put and call, and their prices: the block's mean columns
    at A = 1 without the correlation pair."""
    sq = v * math.sqrt(T)
    d1 = (math.log(X0 / K) + (r - d + 0.5 * v * v) * T) / sq
    d2 = d1 - sq
    pdf = math.exp(-0.5 * d1 * d1) / math.sqrt(2.0 * math.pi)
    eq, er = math.exp(-d * T), math.exp(-r * T)
    vega = X0 * eq * pdf * math.sqrt(T)
    decay = -X0 * eq * pdf * v / (2.0 * math.sqrt(T))
    return [-eq * _ncdf(-d1), eq * _ncdf(d1), vega, vega, -K * T * er * _ncdf(-d2), K * T * er * _ncdf(d2),
            decay + r * K * er * _ncdf(-d2) - d * X0 * eq * _ncdf(-d1),
            decay - r * K * er * _ncdf(d2) + d * X0 * eq * _ncdf(d1),
            K * er * _ncdf(-d2) - X0 * eq * _ncdf(-d1), X0 * eq * _ncdf(d1) - K * er * _ncdf(d2)]


@pytest.mark.parametrize("normalize", [False, True])
def test_reference_single_asset_against_the_closed_form(oracle, normalize) -> None:
    """A = 1: the basket is the asset.  Every Greek within 4 of its own standard errors of the Black-Scholes value, as
    tests/test_gpu_greeks.py::test_greeks_against_the_closed_form asks of the single-asset kernel; correlation is 0."""
    B, T, P = 12, 16, 4096
    rows = cases.contracts(1, B)
    block, sums = gr.greeks(oracle, rows, 1, T, P, SEED, ORD0, normalize=normalize)
    assert block.shape == (B, 24) and sums.shape == (B, 3, 1) and not np.isnan(block).any()
    black = np.array([_black_scholes(*row[[0, 1, 2, 4, 5, 6]]) for row in rows])
    got = block[:, [0, 1, 2, 3, 4, 5, 6, 7, 20, 21]]
    err = block[:, [10, 11, 12, 13, 14, 15, 16, 17, 22, 23]]
    z = np.abs(got - black) / err
    print(f"worst |reference - closed form| / stderr by column: {np.round(z.max(axis=0), 2).tolist()}")
    assert np.all(z <= 4.0), np.argwhere(z > 4.0).tolist()
    assert np.all(block[:, [8, 9, 18, 19]] == 0.0)
    if not normalize:
        assert np.all(sums[:, 1:] == 0.0)


def test_restatement_against_the_reference(oracle) -> None:
    """The float32 restatement of the header's table (portable math, the oracle's kernel-mode terminal values, its own
    float64 sums) against the float64 reference over the contracts of the GPU comparison, per column as a share of the
    column's standard error.  Measured: 1.11e-3 at the most (theta call of (1, 3, 2048, RAW)); no case above 7e-5
    otherwise.  The figure the GPU test allows four times of, cases.MEASURED_SHARE, has to be this measurement (not
    below it, and not above twice it), and four times it has to stay under a quarter of a standard error.  Every
    contract has to pass basket_reference.exercise_count_ok."""
    worst = 0.0
    for A, T, P, norm, B in cases.REFERENCE_CASES:
        rows = cases.sobol_rows(oracle, A, B)
        full = br.reference(oracle, rows, A, T, P, SEED, ORD0, normalize=bool(norm))
        assert br.exercise_count_ok(full.doubt, P), (A, T, P, full.doubt)
        ref, ref_sums = gr.greeks(oracle, rows, A, T, P, SEED, ORD0, normalize=bool(norm))
        n = 4 * A + 6
        # the reference's prices are basket_reference's, and its terminal sums too
        np.testing.assert_allclose(ref[:, 2 * n:2 * n + 2], full.cols[:, :2], rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref[:, 2 * n + 2:], full.cols[:, 6:8], rtol=1e-9, atol=0)
        np.testing.assert_allclose(ref_sums[:, 0], full.tot, rtol=1e-12, atol=0)
        paths, _, _ = oracle.basket_kernel(rows, A, T, 4, -(-P // 2048) * 512, SEED, ordinal0=ORD0, want_paths=True)
        x = np.ascontiguousarray(paths[:, :, -1, :P])
        got = rs.restate(oracle, rows, A, x, norm)
        assert not np.isnan(got["cols"]).any() and not np.isnan(ref).any()
        shares = cases.shares_of_stderr(got["cols"], ref, rows, A)
        col = max(shares, key=shares.get)
        print(f"A {A} T {T} P {P} norm {norm}: largest share of a standard error {shares[col]:.3e} (column {col})")
        worst = max(worst, shares[col])
        # the pass-1 sums: relative to the sum of the magnitudes (sxl and sxc change sign from path to path)
        for q in range(3):
            mag = np.abs([x.astype(np.float64), got["xl"], got["xc"]][q]).sum(axis=2)
            assert np.all(np.abs(got["sums"][:, q] - ref_sums[:, q]) <= 1e-4 * mag), q
    print(f"largest share over all cases {worst:.3e}; allowed on the GPU {cases.ALLOWED_SHARE:.3e}")
    assert cases.MEASURED_SHARE / 2 <= worst <= cases.MEASURED_SHARE
    assert cases.ALLOWED_SHARE == 4 * cases.MEASURED_SHARE <= 0.25
