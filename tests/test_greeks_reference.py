"""The single-asset pathwise Greeks against the independent float64 reference of tests/helpers/greeks_reference.py, on
the CPU: the portable f32 restatement of greeks_kernel (tests/helpers/greeks_restate.py on oracle.kernel_paths, which
tests/test_gpu_greeks.py holds the kernel to) has to lie within the reference's a-priori bound in every column, and
the same formulas in float64 (on oracle.gbm_paths) within the project's float64 tolerance.
tests/test_gpu_greeks_reference.py holds the kernel itself to the same reference, in portable and SMC_MATH_HW math.

The reference is then held to facts it does not share a derivation with: the Black-Scholes closed forms, central
differences of gbm_reference's own Monte-Carlo price on fixed stream words, and the NORMALIZE identities.  The
sensitivity test gives the bound its meaning: each wrong reading of the header's table listed there, put in the
reference's place, has to leave the bound on some case."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest

from tests.helpers import ATOL_FLOAT64, RTOL_FLOAT64, make_domain_bounds
from tests.helpers import gbm_reference as gref
from tests.helpers import gbm_restate as gr
from tests.helpers import greeks_reference as gk
from tests.helpers import greeks_restate as restate

SEED = 7
ORD0 = 11
N_SOBOL = 3
# beside the Sobol-drawn and hand-built rows: T = 0, and a volatility of 1 % where the RAW cancellation in hv = L / v -
# mu T / v - v T is at its worst (both operands near 1 / v times the sum)
EXTRA = {"T 0": (50.0, 40.0, 0.0, 0.1, 0.0, 0.7), "v 0.01": (100.0, 100.5, 1.0, 0.03, 0.01, 0.01)}
# gbm_reference's flat row (X0 = K = 128, r = d, v = 0) has its strike on the v = 0 forward, where every path lies: it
# is the deliberate row of test_strike_on_the_forward_puts_every_path_in_doubt, and the sweep takes it with the strike
# moved off the paths
FLAT = tuple(gref.HAND_BUILT["flat"])


def _oracle():
    import oracle  # noqa: PLC0415

    oracle.build()
    return oracle


@functools.lru_cache(maxsize=None)
def case_rows() -> np.ndarray:
    """Contract rows [14, 6] of every case: three Sobol-drawn rows in the default bounds, gbm_reference's hand-built rows
    (the flat one with its strike at 120, off its paths), the T = 0 row and the v = 0.01 row.
    tests/test_gpu_greeks_reference.py uses the same."""
    lo, hi = make_domain_bounds().arrays()
    hand = gref.hand_built_rows()
    hand[list(gref.HAND_BUILT).index("flat"), 1] = 120.0
    rows = np.concatenate([_oracle().sobol_contracts(SEED, 0, N_SOBOL, lo, hi), hand, np.array(list(EXTRA.values()))])
    rows.setflags(write=False)
    return rows


def degenerate_rows() -> np.ndarray:
    """v = 0, the T v^2 corner, flat (off its paths), T = 0, v = 0.01: the rows whose conventions the header states."""
    rows, names = case_rows(), list(gref.HAND_BUILT)
    pick = [N_SOBOL + names.index(n) for n in ("v 0", "T v^2 corner", "flat")] + [len(rows) - 2, len(rows) - 1]
    return rows[pick]


@functools.lru_cache(maxsize=8)
def _reference(T: int, P: int, normalize: bool) -> gk.GreeksRef:
    return gk.reference(_oracle(), case_rows(), T, P, SEED, ORD0, normalize=normalize)


@functools.lru_cache(maxsize=8)
def _restated(T: int, P: int, normalize: bool) -> np.ndarray:
    _oracle()
    with np.errstate(divide="ignore", invalid="ignore"):
        return restate.block_f32(case_rows(), T, P, SEED, ORD0, int(normalize))


# ---- the sweep -------------------------------------------------------------------------------------------------------
LARGEST: dict[tuple[str, str], float] = {}  # (normalisation, column group) -> the largest share seen so far


@pytest.mark.parametrize("P", [1, 21, 528, 693, 1024, 4096])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 16, 17, 40])
def test_restatement_within_the_bound(T, P) -> None:
    oracle = _oracle()
    rows = case_rows()
    for normalize in (False, True):
        label = f"T {T} P {P} {'NORMALIZE' if normalize else 'RAW'}"
        ref = _reference(T, P, normalize)
        assert gref.count_ok(ref.doubt, P), (label, ref.doubt)  # a condition on the strikes, met by the reference alone
        used = gk.shares(_restated(T, P, normalize), ref)
        r64 = gk.reference(oracle, rows, T, P, SEED, ORD0, normalize=normalize, f64=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            g64 = restate.block_f64(rows, T, P, SEED, ORD0, int(normalize))
        used64 = float(np.max(np.abs(g64 - r64.cols) / gk.tol64(r64, RTOL_FLOAT64, ATOL_FLOAT64)))
        print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
              + f"; f64 share of its tolerance {used64:.2e}; paths in doubt {int(ref.doubt.max())}")
        for kind, v in used.items():
            key = ("NORMALIZE" if normalize else "RAW", kind)
            LARGEST[key] = max(LARGEST.get(key, 0.0), v)
        assert max(used.values()) < 1.0, (label, used)
        assert used64 <= 1.0, (label, used64)
    print("largest share so far: " + ", ".join(f"{n} {k} {v:.3f}" for (n, k), v in sorted(LARGEST.items())))


def test_strike_on_the_forward_puts_every_path_in_doubt() -> None:
    """The deliberate row: no volatility, r = d, K = X0, so every path ends on the strike and either indicator is
    right.  All P paths are in doubt (the count rule of the sweep is a condition this row is built to break), every
    indicator term carries its whole value as error, and the restatement lies inside that."""
    oracle = _oracle()
    rows = np.array([FLAT, FLAT[:1] + (120.0,) + FLAT[2:]])
    T, P = 5, 21
    for normalize in (False, True):
        ref = gk.reference(oracle, rows, T, P, SEED, ORD0, normalize=normalize)
        assert ref.doubt.tolist() == [P, 0]
        assert not gref.count_ok(ref.doubt[:1], P)
        assert np.all(ref.cols[0, [0, 1, 4, 5]] == 0.0)  # strict comparisons: no indicator is set in the reference
        df = math.exp(-0.03)
        assert np.all(ref.bound[0, [0, 1]] >= df) and np.all(ref.bound[0, [4, 5]] >= 128.0 * df)
        assert ref.bound[1, 1] < 1e-5 and ref.bound[1, 5] < 1e-3
        got = restate.block_f32(rows, T, P, SEED, ORD0, int(normalize))
        assert max(gk.shares(got, ref).values()) < 1.0


# ---- sensitivity: wrong readings leave the bound ---------------------------------------------------------------------
RAW, NORM = False, True
# name -> (keyword arguments of greeks_reference.greeks, the normalisations it is a reading of)
MUTANTS = {
    "no -vT in d ln x / d v": ({"no_vT": True}, (RAW,)),
    "aT = mu instead of mu / 2": ({"aT_mu": True}, (RAW,)),
    "theta term off by 1e-4": ({"theta_off": 1e-4}, (RAW,)),
    "no Lbar term": ({"no_lbar": True}, (NORM,)),
    "Lbar as the plain mean": ({"plain_mean": True}, (NORM,)),
    "no (r - d) in the NORMALIZE theta": ({"no_carry_theta": True}, (NORM,)),
    "theta without r payoff": ({"no_r_payoff": True}, (RAW, NORM)),
    "rho with e^{-(r - d) T}": ({"rho_carry": True}, (RAW, NORM)),
    "rho with xs in place of K": ({"rho_xs": True}, (RAW, NORM)),
    "gamma over v T X0": ({"gamma_x0": True}, (RAW, NORM)),
    "indicators exchanged": ({"exchanged": True}, (RAW, NORM)),
    "delta as 1 / K": ({"delta_k": True}, (RAW, NORM)),
    "standard error with P in place of P - 1": ({"stderr_p": True}, (RAW, NORM)),
    "W with dt = T / (steps + 1)": ({"dt_plus": True}, (RAW, NORM)),
}
# Readings that cancel by construction and so cannot be told from the right one: a constant added to d ln x / d v or to
# d ln x / d T under NORMALIZE (the x-weighted mean takes it out again: "no -vT" and "aT = mu" are RAW readings only),
# and 1 / X0 against 1 / K on a contract struck at the money.
# (T, P, normalize): two whole chunks, an odd T with a ragged P, one pass, the stream span, and P = 21 for the n - 1
MUTANT_CASES = [(16, 4096, NORM), (16, 4096, RAW), (5, 693, NORM), (3, 2048, RAW), (1, 528, NORM), (2, 21, RAW), (2, 21, NORM)]


@functools.lru_cache(maxsize=None)
def _mutant_factors() -> dict[str, float]:
    """name -> the largest |restatement - wrong reading| / bound over the case set and the columns."""
    factor = {name: 0.0 for name in MUTANTS}
    for T, P, normalize in MUTANT_CASES:
        good, got = _reference(T, P, normalize), _restated(T, P, normalize)
        assert max(gk.shares(got, good).values()) < 1.0
        for name, (kw, norms) in MUTANTS.items():
            if normalize not in norms or (name.startswith("standard error") and P != 21):
                continue
            with np.errstate(all="ignore"):
                wrong = gk.reference(_oracle(), case_rows(), T, P, SEED, ORD0, normalize=normalize, **kw)
            live = good.bound > 0.0  # a zero bound (a v = 0 vega, an error at P = 1) would turn any miss into infinity
            factor[name] = max(factor[name], gref.share_used(got[live], wrong.cols[live], good.bound[live]))
    return factor


def test_wrong_readings_leave_the_bound() -> None:
    factor = _mutant_factors()
    print("factor by which each wrong reading leaves the bound: " + ", ".join(f"{k}: {v:.3g}" for k, v in factor.items()))
    print(f"the closest: {min(factor, key=factor.get)}")
    assert len(factor) == 14
    survivors = [k for k, v in factor.items() if not v > 1.0]
    assert not survivors, survivors


# ---- the reference against outside facts -----------------------------------------------------------------------------
def _ncdf(x: float) -> float:
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def black_scholes_greeks(X0: float, K: float, T: float, r: float, d: float, v: float) -> list[float]:
    """Columns 0..9 for a European put / call with continuous dividend yield d; theta is -dV/dT per year."""
    sq = v * math.sqrt(T)
    d1 = (math.log(X0 / K) + (r - d + 0.5 * v * v) * T) / sq
    d2 = d1 - sq
    pdf = math.exp(-0.5 * d1 * d1) / math.sqrt(2.0 * math.pi)
    eq, er = math.exp(-d * T), math.exp(-r * T)
    vega = X0 * eq * pdf * math.sqrt(T)
    decay = -X0 * eq * pdf * v / (2.0 * math.sqrt(T))
    gamma = eq * pdf / (X0 * sq)
    return [-eq * _ncdf(-d1), eq * _ncdf(d1), vega, vega, -K * T * er * _ncdf(-d2), K * T * er * _ncdf(d2),
            decay + r * K * er * _ncdf(-d2) - d * X0 * eq * _ncdf(-d1),
            decay - r * K * er * _ncdf(d2) + d * X0 * eq * _ncdf(d1), gamma, gamma]


@pytest.mark.parametrize("normalize", [False, True])
def test_reference_greeks_are_black_scholes(normalize) -> None:
    """Every Greek of the reference within 4 of its own standard errors of the closed form, on the draws of
    tests/test_gpu_greeks.py's closed-form test: 4096 paths of the pricing tests' 12 contracts around the money.  The cap
    is a condition on the draws, not a measurement (the figure is printed).  Under NORMALIZE the errors leave out the
    sampling error of the shared scale and mean (limit 1), so more paths do not keep the ratio down: at
    16384 paths the put theta of one contract lies 4.5 of them out."""
    rows = gr.contracts(12)
    ref = gk.reference(_oracle(), rows, 16, 4096, SEED, ORD0, normalize=normalize)
    black = np.array([black_scholes_greeks(*row) for row in rows.tolist()])
    zs = np.abs(ref.cols[:, :10] - black) / ref.cols[:, 10:20]
    print("worst |reference - closed form| / stderr: " + ", ".join(f"{n} {z:.2f}" for n, z in zip(gk.NAMES, zs.max(axis=0))))
    assert np.all(ref.cols[:, 10:20] > 0.0) and np.all(zs <= 4.0), np.argwhere(zs > 4.0).tolist()


def test_reference_normalize_identities() -> None:
    """NORMALIZE puts the mean of xs on the forward, so call delta - put delta = df F / X0 = e^{-dT} when no path sits on
    the strike; the weights of vega have x-weighted mean zero, so the two vegas are one number; and call rho - put rho =
    T K df.  RAW: the prices and the sum tie to gbm_reference's price columns."""
    oracle = _oracle()
    rows = case_rows()
    for T, P in ((16, 4096), (5, 693), (1, 21)):
        ref = _reference(T, P, True)
        scale = np.abs(ref.cols[:, 2]) + np.abs(ref.cols[:, 3]) + rows[:, 0]
        np.testing.assert_allclose(ref.cols[:, 1] - ref.cols[:, 0], np.exp(-rows[:, 4] * rows[:, 2]), rtol=1e-12)
        assert np.all(np.abs(ref.cols[:, 3] - ref.cols[:, 2]) <= 1e-12 * scale)
        np.testing.assert_allclose(ref.cols[:, 5] - ref.cols[:, 4], rows[:, 2] * rows[:, 1] * np.exp(-rows[:, 3] * rows[:, 2]),
                                   rtol=1e-12)
        for normalize in (False, True):
            price = gref.reference(oracle, rows, T, P, SEED, ORD0, normalize=normalize)
            mine = _reference(T, P, normalize).cols
            np.testing.assert_allclose(mine[:, [20, 21, 22, 23, 24]], price.price[:, [0, 1, 3, 4, 7]], rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize("normalize", [False, True])
def test_reference_greeks_are_derivatives_of_the_price(normalize) -> None:
    """Central differences of gbm_reference's Monte-Carlo put and call (its paths, scaling and payoffs: none of the
    pathwise derivation) in X0, v, r and T on fixed stream words.  The strike of each contract is put in the middle of
    the widest gap between its terminal values near the forward, and the largest step h keeps every path at least
    twice h |d xs / d theta| away from it, so no path crosses the kink and the price is smooth in theta over the
    stencil.  Then the difference quotient converges to the reference's Greek at the O(h^2) rate: over two decades of h
    the error falls by 100 a decade (asked: by 30, down to the f64 noise 1e-16 price / h of the quotient), and at the
    smallest h it is within 1e-6 of the Greek's scale.  In X0 the price is piecewise linear (x and F are proportional to
    X0), so that quotient is exact at every h and only the noise shows."""
    oracle = _oracle()
    T, P = 5, 256
    rows = gr.contracts(6).copy()
    z, rad = gref.normals(gref.stream_words(oracle, rows.shape[0], T, P, SEED, ORD0), T, P)
    xs = np.sort(gk.greeks(rows, T, z, rad, normalize=normalize).xs, axis=1)[:, P // 4:3 * P // 4]
    gaps = np.diff(xs, axis=1)
    at = gaps.argmax(axis=1)
    rows[:, 1] = 0.5 * (xs[np.arange(len(rows)), at] + xs[np.arange(len(rows)), at + 1])
    ref = gk.greeks(rows, T, z, rad, normalize=normalize)
    clear = np.abs(ref.xs - rows[:, 1:2]).min(axis=1)
    worst = 0.0
    for name, column, first, sign in (("X0", 0, 0, 1.0), ("v", 5, 2, 1.0), ("r", 3, 4, 1.0), ("T", 2, 6, -1.0)):
        h0 = clear / (4.0 * np.abs(ref.dxs_dtheta[name]).max(axis=1))
        errs = []
        for k in range(3):
            h = h0 * 10.0 ** -k
            up, dn = rows.copy(), rows.copy()
            up[:, column] += h
            dn[:, column] -= h
            h = (up[:, column] - dn[:, column]) / 2.0  # the step actually taken
            quotient = sign * (gk.prices(up, T, z, normalize) - gk.prices(dn, T, z, normalize)) / (2.0 * h[:, None])
            errs.append(np.abs(quotient - ref.cols[:, first:first + 2]))
        scale = np.abs(ref.cols[:, first:first + 2]).max(axis=1, keepdims=True) + 1e-3
        noise = 64 * 2.0 ** -52 * ref.cols[:, 20:22].max(axis=1, keepdims=True) / (h0[:, None] * 1e-2)
        print(f"{name}: h {h0.min():.2e} .. {h0.max():.2e}, error / scale at h, h / 10, h / 100: "
              + ", ".join(f"{float((e / scale).max()):.2e}" for e in errs))
        assert np.all(errs[1] <= errs[0] / 30.0 + noise), name
        assert np.all(errs[2] <= errs[1] / 30.0 + noise), name
        assert np.all(errs[2] <= 1e-6 * scale), name
        worst = max(worst, float((errs[2] / scale).max()))
    print(f"largest error at the smallest h over the Greek's scale: {worst:.2e}")
