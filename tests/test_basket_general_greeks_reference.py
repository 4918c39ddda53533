"""The float64 reference of the general basket Greeks (tests/helpers/basket_general_greeks_reference.py) held to what it
claims, on the CPU, and the float32 restatement of the header's table (tests/helpers/basket_general_greeks_restate.py)
held to the reference.

1. The reference's Greeks against central differences of basket_general_reference's own Monte-Carlo price on the same
   words (every kind, both normalisations, A in {1, 2, 3, 4, 8}, signed weights among them), with
   tests/test_basket_greeks_reference.py's tolerance: a Richardson estimate, the f64 cancellation, and the paths whose
   exercise changes inside the step.  Wrong readings of the pair columns have to leave that tolerance.
2. With an all-rho matrix and weights 1 / A: the pair columns sum to basket_greeks_reference's correlation column and the
   other columns are its columns, to f64 rounding.
3. Margrabe's closed form for the deltas and the correlation sensitivity of the exchange option.
4. An asset with weight 0 has delta and vega exactly 0.
5. The restatement against the reference, as a share of each column's standard error: the measurement behind the
   tolerance of tests/test_gpu_basket_general_greeks.py."""

from __future__ import annotations

import math

import numpy as np
import pytest

from tests.helpers import basket_general_cases as gcases
from tests.helpers import basket_general_greeks_cases as cases
from tests.helpers import basket_general_greeks_reference as gg
from tests.helpers import basket_general_greeks_restate as rs
from tests.helpers import basket_general_reference as gen
from tests.helpers import basket_greeks_reference as gr
from tests.helpers import basket_reference as br

SEED, ORD0 = cases.SEED, cases.ORD0
REL_STEP = 1e-5
T_FD, P_FD, B_FD = 3, 2048, 4


def _fd_inputs(oracle, A: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Drawn rows, weights and matrices; from A = 2 on the last weight of every other contract is negated (the strike
    is then reset to the weighted forward, kept positive by taking its magnitude)."""
    rows, w, C = gcases.drawn_case(oracle, A, B_FD)
    w = w.copy()
    if A > 1:
        w[::2, -1] *= -1.0
        F = br.forwards(rows, A)[0]
        rows = rows.copy()
        rows[:, 0] = np.abs((w * F).sum(axis=1)) * np.linspace(0.85, 1.2, B_FD)
    return rows, w, C


def _finite_difference_shares(oracle, A: int, normalize: bool, **wrong) -> dict[str, float]:
    """The largest |central difference - pathwise Greek| / tolerance by kind of Greek over the contracts, both payoffs,
    every asset and every pair.  Steps: 1e-5 X0_i, 1e-5 T, and 1e-5 absolute for v_i, r and C_jk (C_jk and C_kj
    together).  The tolerance is tests/test_basket_greeks_reference.py's, from the reference's own values: |D(2h) - D(h)|
    for the truncation, eps_V df (|K| + mean |bk|) / h for the cancellation with eps_V = (T + 16) 2^-52
    (1 + max |ln(x / X0)|), and df |d bk / d theta| / P for every path within 1.5 h |d bk / d theta| of the strike.
    `wrong` is passed to path_terms (the wrong readings); `permute` reorders the pair columns, `inputs` replaces the
    drawn contracts."""
    permute = wrong.pop("permute", None)
    rows, w, C = wrong.pop("inputs", None) or _fd_inputs(oracle, A)
    z = gg.words_and_drivers(oracle, B_FD, A, T_FD, P_FD, SEED, ORD0)
    r = gg.path_terms(rows, A, T_FD, z, w, C, normalize, **wrong)
    block = gg.block_of(r["t"], A)
    pr = gg.pairs(A)
    npr = len(pr)
    if permute is not None:
        for base in (4 * A + 4, 4 * A + 4 + npr):
            block[:, base:base + npr] = block[:, base:base + npr][:, permute]
    K, Tm, _, _, X0, _, _ = br.fields(rows, A)
    eps_v = (T_FD + 16) * 2.0 ** -52 * (1.0 + np.abs(np.log(r["xT"] / X0[:, :, None])).max(axis=(1, 2)))
    scale = r["df"] * (np.abs(K) + np.abs(r["bk"]).mean(axis=1))
    one = np.full(B_FD, REL_STEP)

    def bump_row(field):
        def apply(step):
            up, down = rows.copy(), rows.copy()
            up[:, field] += step
            down[:, field] -= step
            return (up, C), (down, C)
        return apply

    def bump_pair(j, k):
        def apply(step):
            up, down = C.copy(), C.copy()
            for a, s in ((up, step), (down, -step)):
                a[:, j, k] += s
                a[:, k, j] += s
            return (rows, up), (rows, down)
        return apply

    # (kind, bump, put column, call column, step, sign of the reported Greek)
    params = [("delta", bump_row(4 + i), i, A + i, REL_STEP * X0[:, i], 1.0) for i in range(A)]
    params += [("vega", bump_row(4 + 2 * A + i), 2 * A + i, 3 * A + i, one, 1.0) for i in range(A)]
    params += [("rho", bump_row(2), 4 * A, 4 * A + 1, one, 1.0), ("theta", bump_row(1), 4 * A + 2, 4 * A + 3, REL_STEP * Tm, -1.0)]
    params += [("pair", bump_pair(j, k), 4 * A + 4 + q, 4 * A + 4 + npr + q, one, 1.0) for q, (j, k) in enumerate(pr)]
    used: dict[str, float] = {}
    for index, (kind, bump, put_col, call_col, h, sign) in enumerate(params):
        def quotient(step: np.ndarray) -> np.ndarray:
            (ru, cu), (rd, cd) = bump(step)
            return sign * (gg.prices(ru, A, T_FD, z, w, cu, normalize) - gg.prices(rd, A, T_FD, z, w, cd, normalize)) \
                / (2 * step[:, None])

        d1, d2 = quotient(h), quotient(2 * h)
        slope = np.abs(r["dbk"][index])
        crossing = np.abs(K[:, None] - r["bk"]) <= 1.5 * h[:, None] * slope
        kink = (crossing * r["df"][:, None] * slope).sum(axis=1) / P_FD
        tol = np.abs(d2 - d1) + (kink + eps_v * scale / h)[:, None]
        err = np.abs(d1 - block[:, [put_col, call_col]])
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0.0, 0.0, err / tol)
        used[kind] = max(used.get(kind, 0.0), float(np.where(np.isnan(share), np.inf, share).max()))
    return used


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 8])
def test_reference_greeks_are_the_derivatives_of_the_general_price(oracle, A, normalize) -> None:
    used = _finite_difference_shares(oracle, A, normalize)
    print(f"A {A} {'NORMALIZE' if normalize else 'RAW'}: share of the tolerance used " +
          ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert set(used) == {"delta", "vega", "rho", "theta"} | ({"pair"} if A > 1 else set())
    assert max(used.values()) < 1.0, used


def _half(L, j, k):
    return 0.5 * gg.dfactor_pair(L, j, k)


def _transposed(L, j, k):
    G = gg.dfactor_pair(L, j, k) @ np.linalg.inv(L)
    return G.T @ L


def _phi_for_g(L, j, k):
    Li = np.linalg.inv(L)
    E = np.zeros_like(L)
    E[j, k] = E[k, j] = 1.0
    S = Li @ E @ Li.T
    return (np.tril(S, -1) + 0.5 * np.diag(np.diag(S))) @ L


def test_wrong_readings_leave_the_tolerance(oracle) -> None:
    """Each wrong reading is off on the columns it touches, and only there; the smallest factor by which one leaves
    the tolerance is printed."""
    A = 4
    col_major = [gg.pairs(A).index(p) for p in sorted(gg.pairs(A), key=lambda jk: (jk[1], jk[0]))]
    assert col_major != list(range(6))
    readings = [("the triangle read column-major", dict(permute=col_major), ("pair",), (False, True)),
                ("only C_jk bumped, not C_kj", dict(dfactor=_half), ("pair",), (False, True)),
                ("G transposed", dict(dfactor=_transposed), ("pair",), (False, True)),
                ("Phi(S) used for G", dict(dfactor=_phi_for_g), ("pair",), (False, True)),
                ("ac dropped", dict(drop_ac=True), ("pair",), (True,))]
    least = np.inf
    for what, kw, touched, norms in readings:
        for normalize in norms:
            used = _finite_difference_shares(oracle, A, normalize, **dict(kw))
            print(f"{what}, {'NORMALIZE' if normalize else 'RAW'}: share of the tolerance used {used}")
            assert all(used[k] > 1.0 for k in touched), (what, used)
            assert max(v for k, v in used.items() if k not in touched) < 1.0, (what, used)
            least = min(least, min(used[k] for k in touched))
    # |w_i| on a spread: the exchange option's terms with the magnitudes of the weights; rho does not see the weights
    spread = gcases.spread_case(oracle, B_FD)
    for normalize in (False, True):
        assert max(_finite_difference_shares(oracle, 2, normalize, inputs=spread).values()) < 1.0
        used = _finite_difference_shares(oracle, 2, normalize, inputs=spread, term_weights=np.abs(spread[1]))
        print(f"|w| on a spread, {'NORMALIZE' if normalize else 'RAW'}: share of the tolerance used {used}")
        touched = ("delta", "vega", "theta", "pair")
        assert all(used[k] > 1.0 for k in touched) and used["rho"] < 1.0, used
        least = min(least, min(used[k] for k in touched))
    print(f"the smallest factor by which a wrong reading leaves the finite-difference tolerance: {least:.1f}")
    assert least > 2.0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 8])
def test_chain_rule_against_the_equicorrelation_reference(oracle, A, normalize) -> None:
    B, T, P = 3, 3, 512
    rows = gcases.sobol_rows(oracle, A, B)
    old, old_sums = gr.greeks(oracle, rows, A, T, P, SEED, ORD0, normalize=normalize)
    new, sums = gg.greeks(oracle, rows, A, T, P, SEED, ORD0, normalize=normalize)
    explicit, _ = gg.greeks(oracle, rows, A, T, P, SEED, ORD0, weights=np.full(A, 1.0 / A),
                            corr=gg.matrices(rows, A, None), normalize=normalize)
    np.testing.assert_array_equal(new, explicit)
    npr, n, m = A * (A - 1) // 2, gg.greek_columns(A), 4 * A + 6
    scale = np.abs(old).max(axis=1, keepdims=True)
    assert np.all(np.abs(new[:, :4 * A + 4] - old[:, :4 * A + 4]) <= 1e-12 * scale)
    assert np.all(np.abs(new[:, n:n + 4 * A + 4] - old[:, m:m + 4 * A + 4]) <= 1e-12 * scale)
    assert np.all(np.abs(new[:, 2 * n:] - old[:, 2 * m:]) <= 1e-12 * scale)
    for side in range(2):
        pair_sum = new[:, 4 * A + 4 + side * npr:4 * A + 4 + (side + 1) * npr].sum(axis=1)
        assert np.all(np.abs(pair_sum - old[:, 4 * A + 4 + side]) <= 1e-10 * scale[:, 0])
    np.testing.assert_allclose(sums[:, :A], old_sums[:, 0], rtol=1e-13)
    diag = [A + i * (i + 1) // 2 + i for i in range(A)]
    if normalize:  # M_ii from the drivers against sum x ln(x / X0) from the terminal values
        np.testing.assert_allclose(sums[:, diag], old_sums[:, 1], rtol=1e-9, atol=1e-9 * np.abs(old_sums[:, 0]).max())
    else:
        assert np.all(sums[:, A:] == 0.0)


def test_margrabe_deltas_and_correlation_sensitivity(oracle) -> None:
    """The 32 exchange options under RAW: both deltas and dV / drho = -X_1 e^{-d_1 T} phi(d_1) sqrt(T) v_1 v_2 / sigma,
    within 5 of the reference's own standard errors (the price test's multiple)."""
    rows = gcases.margrabe_rows()
    T, P = gcases.MARGRABE["T"], gcases.MARGRABE["P"]
    ref, _ = gg.greeks(oracle, rows, 2, T, P, SEED, ORD0, weights=np.array([1.0, -1.0]), normalize=False)
    _, Tm, r, rho, X0, d, v = br.fields(rows, 2)
    sig = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2 - 2.0 * rho * v[:, 0] * v[:, 1])
    F = X0 * np.exp((r[:, None] - d) * Tm[:, None])
    d1 = (np.log(F[:, 0] / F[:, 1]) + 0.5 * sig * sig * Tm) / (sig * np.sqrt(Tm))
    Phi = lambda a: 0.5 * (1.0 + np.array([math.erf(t / math.sqrt(2.0)) for t in a]))  # noqa: E731
    want = np.stack([np.exp(-d[:, 0] * Tm) * Phi(d1), -np.exp(-d[:, 1] * Tm) * Phi(d1 - sig * np.sqrt(Tm)),
                     -X0[:, 0] * np.exp(-d[:, 0] * Tm) * np.exp(-0.5 * d1 * d1) / np.sqrt(2.0 * np.pi) * np.sqrt(Tm)
                     * v[:, 0] * v[:, 1] / sig], axis=1)
    n = gg.greek_columns(2)
    cols = [2, 3, 13]
    z = np.abs(ref[:, cols] - want) / ref[:, [c + n for c in cols]]
    print(f"worst |reference - Margrabe| / stderr (delta 0, delta 1, correlation): {np.round(z.max(axis=0), 2).tolist()}")
    assert np.all(z <= 5.0), np.argwhere(z > 5.0).tolist()
    np.testing.assert_allclose(ref[:, 2 * n + 1], gen.margrabe(rows), rtol=0, atol=5.0 * ref[:, 2 * n + 3].max())


@pytest.mark.parametrize("normalize", [False, True])
def test_zero_weight_gives_exact_zeros(oracle, normalize) -> None:
    A, B, T, P = 3, 3, 3, 512
    rows, w, C = gcases.drawn_case(oracle, A, B)
    w = w.copy()
    w[:, 1] = 0.0
    ref, _ = gg.greeks(oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=normalize)
    n = gg.greek_columns(A)
    for col in (1, A + 1, 2 * A + 1, 3 * A + 1):
        assert np.all(ref[:, col] == 0.0) and np.all(ref[:, n + col] == 0.0)
    assert not np.isnan(ref).any()


def test_restatement_against_the_reference(oracle) -> None:
    """The float32 restatement against the float64 reference over the contracts of the GPU comparison, per column as a
    share of the column's standard error.  Measured on the CPU: 2.34e-5 at the most (the put price of (1, 3, 2047,
    RAW)).  cases.MEASURED_SHARE has to be this measurement (not below it, and not above twice it); the GPU test allows
    four times it, 1.0e-4, which has to stay under a quarter of a standard error.  On the MI355X the largest share
    was 2.70e-5 (hw math, A = 8, T = 1, P = 4109, replay; portable 2.34e-5).  Every contract has to pass
    basket_reference.exercise_count_ok, and the reference's prices have to be basket_general_reference's."""
    worst = 0.0
    for kind, A, T, P, norm, B in cases.REFERENCE_CASES:
        rows, w, C = cases.inputs(kind, A, B)
        full = gen.reference(oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=bool(norm))
        assert br.exercise_count_ok(full.doubt, P), (kind, A, T, P, full.doubt)
        ref, ref_sums = gg.greeks(oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=bool(norm))
        n = gg.greek_columns(A)
        np.testing.assert_allclose(ref[:, 2 * n:2 * n + 2], full.cols[:, :2], rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref[:, 2 * n + 2:], full.cols[:, 6:8], rtol=1e-9, atol=0)
        np.testing.assert_allclose(ref_sums[:, :A], full.tot, rtol=1e-12, atol=0)
        x = rs.terminal_values(oracle, rows, A, T, P, SEED, ORD0, C)
        np.testing.assert_allclose(x.astype(np.float64), full.xT, rtol=1e-4)
        got = rs.restate(oracle, rows, A, x, w, C, bool(norm))
        assert not np.isnan(got).any() and not np.isnan(ref).any()
        shares = cases.shares_of_stderr(got, ref, rows, A)
        col = max(shares, key=shares.get)
        print(f"{kind} A {A} T {T} P {P} norm {norm}: largest share of a standard error {shares[col]:.3e} (column {col})")
        worst = max(worst, shares[col])
    print(f"largest share over all cases {worst:.3e}; allowed on the GPU {cases.ALLOWED_SHARE:.3e}")
    assert cases.MEASURED_SHARE / 2 <= worst <= cases.MEASURED_SHARE
    assert cases.ALLOWED_SHARE == 4 * cases.MEASURED_SHARE <= 0.25
