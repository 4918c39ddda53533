"""The independent reference of smc_basket_greeks_paths (tests/helpers/basket_path_greeks_reference.py) on the CPU:
its Greeks are the central differences of basket_path_reference's own f64 prices on common drivers; at T = 1 they are
basket_general_greeks_reference's, at A = 1 path_greeks_reference's; a zero weight gives exact zeros; the caps on the
inputs of the bound tests hold for every case before any device output exists; and named wrong readings leave the
bound.  No device, no library call."""

from __future__ import annotations

import numpy as np
import pytest

from tests.helpers import basket_general_greeks_reference as gg
from tests.helpers import basket_path_greeks_cases as gc
from tests.helpers import basket_path_greeks_reference as pg
from tests.helpers import basket_path_reference as bp
from tests.helpers import basket_reference as br
from tests.helpers import gbm_reference as gref
from tests.helpers import path_greeks_reference as pgr

SEED, ORD0 = gc.SEED, gc.ORD0
REL_STEP = 1e-5
T_FD, P_FD, B_FD = 3, 1024, 4


@pytest.fixture(scope="module")
def oracle():
    import oracle as _oracle

    _oracle.build()
    return _oracle


def _finite_difference_shares(oracle, A: int, normalize: bool, spread: bool = False) -> dict[str, float]:
    """The largest |central difference - pathwise Greek| / tolerance by kind of Greek over the contracts, the four
    payoffs and every asset.  Steps: 1e-5 X0_i, 1e-5 T, and 1e-5 absolute for v_i and r.  The tolerance is
    tests/test_basket_general_greeks_reference.py's rule, from the reference's own values: |D(2h) - D(h)| for the
    truncation, eps_V df (|K| + mean |u|) / h for the cancellation with eps_V = (T + 16) 2^-52 (1 + max |ln(x / X0)|),
    and for the kinks every path whose exercise or whose row of an extreme differs between the two outer bumps
    (+-2h) is charged its whole quotient and its whole pathwise term, over P."""
    rows, w, C = gc.inputs(A, B_FD, spread)
    Lf = np.linalg.cholesky(C)
    z, rad = pg.draws(oracle, rows, A, T_FD, P_FD, SEED, ORD0)
    ref = pg.greeks(rows, A, T_FD, z, rad, w, Lf, normalize=normalize)
    base = pg.path_payoffs(rows, A, T_FD, z, rad, w, Lf, normalize)
    np.testing.assert_allclose(base["pay"].mean(axis=2).T, pg.prices(rows, A, T_FD, z, rad, w, Lf, normalize), rtol=1e-12)
    K, Tm, r, _, X0, _, _ = br.fields(rows, A)
    x, _ = br.paths(rows, A, T_FD, z, rad, br.PORTABLE, L=Lf)
    eps_v = (T_FD + 16) * 2.0 ** -52 * (1.0 + np.abs(np.log(x / X0[:, :, None, None])).max(axis=(1, 2, 3)))
    df = np.exp(-r * Tm)
    scale = df[None, :] * (np.abs(K)[None, :] + np.abs(base["under"]).mean(axis=2))       # [4, B]
    one = np.full(B_FD, REL_STEP)
    params = [("delta", 4 + i, i, REL_STEP * X0[:, i], 1.0) for i in range(A)]
    params += [("vega", 4 + 2 * A + i, A + i, one, 1.0) for i in range(A)]
    params += [("rho", 2, 2 * A, one, 1.0), ("theta", 1, 2 * A + 1, REL_STEP * Tm, -1.0)]
    used: dict[str, float] = {}
    for kind, field, g, h, sign in params:
        def bumped(step: np.ndarray):
            up, down = rows.copy(), rows.copy()
            up[:, field] += step
            down[:, field] -= step
            return (pg.path_payoffs(rows_, A, T_FD, z, rad, w, Lf, normalize) for rows_ in (up, down))

        u1, d1 = bumped(h)
        u2, d2 = bumped(2 * h)
        q1 = sign * (u1["pay"] - d1["pay"]) / (2 * h[None, :, None])                     # [4, B, P]
        q2 = sign * (u2["pay"] - d2["pay"]) / (4 * h[None, :, None])
        kinked = (u2["pay"] > 0) != (d2["pay"] > 0)
        moved = u2["rows_at"] != d2["rows_at"]
        kinked[2] |= moved[0]
        kinked[3] |= moved[1]
        term = ref.terms[g]                                                               # [4, B, P]
        kink = (kinked * (np.abs(q1) + np.abs(term))).sum(axis=2) / P_FD
        D1, D2 = q1.mean(axis=2), q2.mean(axis=2)
        tol = np.abs(D2 - D1) + kink + (eps_v[None, :] * scale) / h[None, :]
        err = np.abs(D1 - np.stack([ref.cols[:, pg.column(A, g, q)] for q in range(4)]))
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0.0, 0.0, err / tol)
        used[kind] = max(used.get(kind, 0.0), float(np.where(np.isnan(share), np.inf, share).max()))
    return used


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 8])
def test_reference_greeks_are_the_derivatives_of_the_path_price(oracle, A, normalize) -> None:
    used = _finite_difference_shares(oracle, A, normalize)
    print(f"A {A} {'NORMALIZE' if normalize else 'RAW'}: share of the tolerance used " +
          ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert set(used) == {"delta", "vega", "rho", "theta"}
    assert max(used.values()) < 1.0, used


@pytest.mark.parametrize("normalize", [False, True])
def test_reference_greeks_of_the_spread(oracle, normalize) -> None:
    used = _finite_difference_shares(oracle, 2, normalize, spread=True)
    print(f"spread {'NORMALIZE' if normalize else 'RAW'}: share of the tolerance used {used}")
    assert max(used.values()) < 1.0, used


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A", [1, 3, 8])
def test_one_time_step_is_the_general_reference(oracle, A, normalize) -> None:
    """T = 1: the average and both extremes are the terminal level, so every Greek of all four payoffs is
    basket_general_greeks_reference's delta, vega, rho and theta to f64 rounding."""
    B, P = 4, 693
    rows, w, C = gc.inputs(A, B)
    ref = pg.reference(oracle, rows, A, 1, P, SEED, ORD0, weights=w, corr=C, normalize=normalize)
    eref, _ = gg.greeks(oracle, rows, A, 1, P, SEED, ORD0, weights=w, corr=C, normalize=normalize)
    n = gg.greek_columns(A)
    for g in range(pg.kinds(A)):
        for q in range(4):
            side = q & 1
            e = (2 * (g // A) + side) * A + g % A if g < 2 * A else 4 * A + 2 * (g - 2 * A) + side
            np.testing.assert_allclose(ref.cols[:, pg.column(A, g, q)], eref[:, e], rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(ref.cols[:, pg.column(A, g, q, True)], eref[:, n + e], rtol=1e-9, atol=1e-11)
    for q in range(4):
        np.testing.assert_allclose(ref.cols[:, pg.column(A, pg.kinds(A), q)], eref[:, 2 * n + (q & 1)], rtol=1e-12)


@pytest.mark.parametrize("normalize", [False, True])
def test_one_asset_restates_the_single_asset_reference(oracle, normalize) -> None:
    """A = 1, weight 1: the model of tests/helpers/path_greeks_reference.py on the same normals."""
    B, T, P = 4, 5, 693
    rows, _, _ = gc.inputs(1, B)
    z, rad = pg.draws(oracle, rows, 1, T, P, SEED, ORD0)
    ref = pg.greeks(rows, 1, T, z, rad, np.ones((B, 1)), np.ones((B, 1, 1)), normalize=normalize)
    K, Tm, r, _, X0, d, v = br.fields(rows, 1)
    single = np.column_stack([X0[:, 0], K, Tm, r, d[:, 0], v[:, 0]])
    assert gref.fields(single)[0] is not None
    sref = pgr.greeks(single, T, z[:, 0], rad[:, 0], "portable", normalize=normalize)
    assert ref.cols.shape == sref.cols.shape == (B, 40)
    np.testing.assert_allclose(ref.cols, sref.cols, rtol=1e-9, atol=1e-11)


def test_a_zero_weight_gives_exact_zeros(oracle) -> None:
    A, B, T, P = 3, 4, 4, 693
    rows, w, C = gc.inputs(A, B)
    w = w.copy()
    w[:, 1] = 0.0
    for normalize in (False, True):
        ref = pg.reference(oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=normalize)
        for g in (1, A + 1):
            for q in range(4):
                assert np.all(ref.cols[:, pg.column(A, g, q)] == 0.0)
                assert np.all(ref.cols[:, pg.column(A, g, q, True)] == 0.0)
        assert np.any(ref.cols[:, pg.column(A, 0, 0)] != 0.0)


@pytest.mark.parametrize("case", gc.CASES + [gc.SPREAD], ids=lambda c: f"A{c[0]}-T{c[1]}-P{c[2]}")
def test_the_caps_hold_for_every_case(oracle, case) -> None:
    """The conditions the GPU bound tests state on their inputs, on the reference alone: few paths whose exercise
    indicator or whose row of an extreme the bound leaves open, in both maths and both normalisations."""
    A, T, P, B = case
    for math in gc.MATHS:
        for normalize in (True, False):
            ref = gc.reference(oracle, A, T, P, B, math, normalize, case is gc.SPREAD)
            assert gref.count_ok(ref.doubt_ind, P), (math, normalize, ref.doubt_ind)
            assert pgr.arg_ok(ref.doubt_arg, P), (math, normalize, ref.doubt_arg)
            assert np.all(np.isfinite(ref.cols)) and np.all(np.isfinite(ref.bound))
            G = pg.kinds(A)
            # the bound is not vacuous: every Greek's bound is below its own standard error
            se = ref.cols[:, 4 * G:8 * G]
            assert np.all(ref.bound[:, :4 * G] < se + 1e-300 * (se == 0)), (math, normalize)


# (wrong reading, case, spread, normalisations, Greek kind as a function of A, payoffs)
WRONG_READINGS = [
    ("no_lbar", (3, 5, 2048, 6), False, (True,), lambda A: A, (0, 1, 2, 3)),
    ("terminal_tau", (3, 5, 2048, 6), False, (True, False), lambda A: 2 * A, (0, 1, 2, 3)),
    ("maturity_only", (3, 5, 2048, 6), False, (True, False), lambda A: 2 * A + 1, (0, 1)),
    ("vega_cross", (3, 5, 2048, 6), False, (True, False), lambda A: A, (0, 1, 2, 3)),
    ("abs_w", gc.SPREAD, True, (True, False), lambda A: 1, (0, 1, 2, 3)),
    ("over_T1", (3, 5, 2048, 6), False, (True, False), lambda A: 0, (0, 1)),
]


@pytest.mark.parametrize("what,case,spread,norms,kind,payoffs", WRONG_READINGS, ids=[w[0] for w in WRONG_READINGS])
def test_wrong_readings_leave_the_bound(oracle, what, case, spread, norms, kind, payoffs) -> None:
    """Each wrong reading moves at least half the contracts of its case out of the bound of a named column: Lbar
    dropped (vega_0), the terminal tau on every row (rho), only the maturity moving with T (theta of the Asian pair),
    vega_j charged to asset i (vega_0), |w| on the spread (delta_1), the average over T + 1 (delta_0 of the Asian
    pair)."""
    A, T, P, B = case
    rows, w, C = gc.inputs(A, B, spread)
    z, rad = gc.draws(oracle, A, T, P, B, spread)
    for normalize in norms:
        ref = gc.reference(oracle, A, T, P, B, "portable", normalize, spread)
        bad = pg.greeks(rows, A, T, z, rad, w, np.linalg.cholesky(C), normalize=normalize, **{what: True})
        for q in payoffs:
            col = pg.column(A, kind(A), q)
            out = np.abs(bad.cols[:, col] - ref.cols[:, col]) > ref.bound[:, col]
            print(f"{what} {'NORMALIZE' if normalize else 'RAW'} column {col}: {int(out.sum())} of {B} contracts out")
            assert 2 * out.sum() >= B, (what, normalize, q)


def test_the_last_row_winning_a_tie_leaves_the_bound(oracle) -> None:
    """Rows tie only where they are equal: the flat contract (every v_i = 0, r = d_i).  The last row in place of the
    first moves rho of both lookback payoffs out of the bound."""
    A, T, P = 3, 4, 693
    rows, w, C = gc.flat_inputs(A)
    z, rad = pg.draws(oracle, rows, A, T, P, SEED, ORD0)
    for normalize in (True, False):
        ref = pg.greeks(rows, A, T, z, rad, w, np.linalg.cholesky(C), normalize=normalize)
        bad = pg.greeks(rows, A, T, z, rad, w, np.linalg.cholesky(C), normalize=normalize, last_tie=True)
        col = pg.column(A, 2 * A, 3)  # the call is in the money: b = mean X0 > K
        assert np.all(np.abs(bad.cols[:, col] - ref.cols[:, col]) > ref.bound[:, col])
        np.testing.assert_array_equal(bad.cols[:, pg.column(A, 2 * A, 0)], ref.cols[:, pg.column(A, 2 * A, 0)])
