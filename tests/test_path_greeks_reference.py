"""The independent reference of smc_gbm_greeks_paths (tests/helpers/path_greeks_reference.py) on the CPU: the portable
f32 restatement (tests/helpers/path_greeks_restate.py) lies within its a-priori bound, the inputs of the bound tests
keep the bound from being vacuous (indicators and extreme rows in doubt under their caps), each of a list of wrong
readings leaves the bound on a named column, and every path's term agrees with the central difference of the
reference's own payoff on the same normals.  No GPU."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import oracle as _oracle
from tests.helpers import gbm_reference as gref
from tests.helpers import path_greeks_reference as pg
from tests.helpers import path_greeks_restate as restate
from tests.helpers.path_greeks_cases import CASES, FLAT_ROWS, ORD0, ROWS, SEED


@functools.lru_cache(maxsize=None)
def _ref(T: int, P: int, norm: int, math: str = "portable") -> pg.PathGreeksRef:
    _oracle.build()
    return pg.reference(_oracle, ROWS, T, P, SEED, ORD0, math=math, normalize=bool(norm))


@functools.lru_cache(maxsize=None)
def _restated(T: int, P: int, norm: int) -> np.ndarray:
    return restate.block_f32(ROWS, T, P, SEED, ORD0, norm)


@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("T,P", CASES)
def test_restatement_within_the_bound_and_the_caps_hold(T, P, norm) -> None:
    ref = _ref(T, P, norm)
    got = _restated(T, P, norm)
    assert np.isfinite(ref.cols).all() and np.isfinite(ref.bound).all()
    print(f"T {T} P {P} norm {norm}: indicators in doubt {ref.doubt_ind.tolist()}, rows in doubt {ref.doubt_arg.tolist()}")
    assert gref.count_ok(ref.doubt_ind, P) and pg.arg_ok(ref.doubt_arg, P)
    for math in ("hw", "f64"):  # the inputs meet the caps in the other typings as well
        if math == "f64" and not gref.LONGDOUBLE_OK:
            continue
        other = _ref(T, P, norm, math)
        assert gref.count_ok(other.doubt_ind, P) and pg.arg_ok(other.doubt_arg, P), math
    for name, cols in (("means", pg.MEAN_COLS), ("stderr", pg.STDERR_COLS)):
        share = gref.share_used(got[:, cols], ref.cols[:, cols], ref.bound[:, cols])
        print(f"  {name}: largest share of the bound {share:.3f}")
        assert share <= 1.0, name
    rel = ref.bound[:, pg.MEAN_COLS] / np.maximum(np.abs(ref.cols[:, pg.MEAN_COLS]), 1e-300)
    print(f"  the bounds of the mean columns: median {np.median(rel):.2e} of the column, largest {rel.max():.2e}")


# (wrong reading, normalisation, column, rows): the column where the reading must leave the bound
SENSITIVITY = [
    ("no_lbar", 1, pg.column(1, 1), "regular"),          # Asian call vega without Lbar's share
    ("plain_mean", 1, pg.column(1, 1), "regular"),       # a plain mean instead of the x-weighted one
    ("terminal_tau", 0, pg.column(2, 1), "regular"),     # Asian call rho with tau = T on every row
    ("terminal_tau", 1, pg.column(2, 3), "regular"),     # lookback call rho likewise
    ("last_tie", 0, pg.column(2, 3), "flat"),            # lookback call rho on the flat row: the last row's tau
    ("maturity_only", 0, pg.column(3, 1), "regular"),    # Asian call theta with the maturity alone moving
    ("maturity_only", 1, pg.column(3, 1), "regular"),
    ("rho_no_discount", 0, pg.column(2, 0), "regular"),  # Asian put rho without -T put
    ("with_x0", 0, pg.column(0, 1), "regular"),          # Asian call delta with X0 monitored
    ("with_x0", 1, pg.column(4, 1), "regular"),          # Asian call price likewise
    ("exchanged", 0, pg.column(4, 3), "regular"),        # lookback call on the minimum
    ("exchanged", 1, pg.column(1, 2), "regular"),        # lookback put vega on the maximum
]


@pytest.mark.parametrize("wrong,norm,col,which", SENSITIVITY)
def test_a_wrong_reading_leaves_the_bound(wrong, norm, col, which) -> None:
    T, P = 5, 693
    _oracle.build()
    if which == "flat":
        crows = FLAT_ROWS
        got = restate.block_f32(crows, T, P, SEED, ORD0, norm)
        right = pg.reference(_oracle, crows, T, P, SEED, ORD0, normalize=bool(norm))
        assert not right.doubt_arg.any() and not right.doubt_ind.any()
        for c in (pg.column(0, 1), pg.column(0, 3)):  # the flat row's deltas are within the bound as well
            assert np.all(np.abs(got[:, c] - right.cols[:, c]) <= right.bound[:, c])
    else:
        crows, got, right = ROWS, _restated(T, P, norm), _ref(T, P, norm)
    bad = pg.reference(_oracle, crows, T, P, SEED, ORD0, normalize=bool(norm), **{wrong: True})
    rows = list(range(len(crows)))
    assert np.all(np.abs(got[rows, col] - right.cols[rows, col]) <= right.bound[rows, col])
    excess = np.abs(got[rows, col] - bad.cols[rows, col]) / bad.bound[rows, col]
    print(f"{wrong} norm {norm} column {col}: smallest distance {excess.min():.1f} bounds")
    assert np.all(excess > 1.0), (wrong, col, excess)


# ---- finite differences of the reference's own payoff ------------------------------------------------------------------
H_REL = 1e-4            # the bump: H_REL of X0, v and T, and H_REL absolute in r
FD_MULTIPLE = 4.0       # the central difference's h^2 error is 4/3 of |FD(h) - FD(h / 2)|; three times that


@pytest.mark.parametrize("norm", [0, 1])
def test_terms_agree_with_central_differences_of_the_reference_payoff(norm) -> None:
    T, P = 5, 693
    _oracle.build()
    rows = ROWS.copy()
    z, rad = pg.draws(_oracle, rows, T, P, SEED, ORD0)
    ref = pg.greeks(rows, T, z, rad, normalize=bool(norm))
    base = pg.payoffs(rows, T, z, bool(norm))
    worst_share, least_compared = 0.0, 1.0
    for g, (field, sign) in enumerate(((0, 1.0), (5, 1.0), (3, 1.0), (2, -1.0))):   # X0, v, r, T; theta = -d/dT
        h = H_REL * (np.ones(len(rows)) if field == 3 else rows[:, field])

        def at(step):
            bumped = rows.copy()
            bumped[:, field] += step * h
            return pg.payoffs(bumped, T, z, bool(norm))

        runs = {s: at(s) for s in (-1.0, -0.5, 0.5, 1.0)}
        fd1 = (runs[1.0]["pay"] - runs[-1.0]["pay"]) / (2 * h[None, :, None])
        fd2 = (runs[0.5]["pay"] - runs[-0.5]["pay"]) / (h[None, :, None])
        K = rows[:, 1][None, :, None]
        for q in range(4):
            fam = 0 if q < 2 else (1 if q == 2 else 2)   # average, minimum, maximum
            keep = np.ones((len(rows), P), dtype=bool)
            for run in list(runs.values()) + [base]:
                keep &= (run["under"][fam] > K[0]) == (base["under"][fam] > K[0])
                if fam:
                    keep &= run["rows_at"][fam - 1] == base["rows_at"][fam - 1]
            want = sign * fd1[q]
            floor = 64 * 2.0 ** -53 * (np.abs(base["under"][fam]) + K[0]) / h[:, None]
            tol = FD_MULTIPLE * np.abs(fd1[q] - fd2[q]) + floor
            err = np.abs(ref.terms[g, q] - want)
            assert np.all(err[keep] <= tol[keep]), (pg.GREEKS[g], pg.PAYOFFS[q], float((err / tol)[keep].max()))
            worst_share = max(worst_share, float((err / tol)[keep].max()))
            least_compared = min(least_compared, float(keep.mean()))
            # the comparison has teeth: the tolerance is small against the term where it is live
            live = keep & (np.abs(want) > 0)
            assert np.median(tol[live] / np.abs(want[live])) < 1e-5
    print(f"norm {norm}: largest share of the tolerance {worst_share:.3f}, least share of paths compared {least_compared:.3f}")
    assert least_compared >= 0.9
