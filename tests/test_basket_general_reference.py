"""tests/helpers/basket_general_reference.py on the CPU: with equal weights and the equicorrelation factor it is
tests/helpers/basket_reference.py; its correlation is right (the Margrabe exchange option, a closed form in rho);
and wrong readings of the new inputs leave its bound, which is what gives tests/test_gpu_basket_general.py teeth."""

from __future__ import annotations

import numpy as np
import pytest

import oracle as _oracle
from tests.helpers import basket_general_cases as cases
from tests.helpers import basket_general_reference as gr
from tests.helpers import basket_reference as br

SEED, ORD0 = cases.SEED, cases.ORD0


@pytest.fixture(scope="module")
def case_4_16_4096():
    """The (4, 16, 4096) case of the GPU test and its reference."""
    A, T, P, norm, B = cases.CASES[0]
    rows, w, C = cases.drawn_case(_oracle, A, B)
    ref = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=bool(norm))
    assert br.exercise_count_ok(ref.doubt, P), ref.doubt
    return rows, w, C, ref


@pytest.mark.parametrize("A,T,P", [(1, 3, 693), (3, 5, 2048), (4, 16, 2049), (8, 2, 1024)])
@pytest.mark.parametrize("normalize", [True, False])
def test_equal_weights_and_equicorrelation_give_the_existing_reference(A, T, P, normalize) -> None:
    rows = cases.sobol_rows(_oracle, A, 4)
    old = br.reference(_oracle, rows, A, T, P, SEED, ORD0, normalize=normalize)
    _, _, _, rho, _, _, _ = br.fields(rows, A)
    C = np.stack([(1.0 - rh) * np.eye(A) + rh * np.ones((A, A)) for rh in rho])
    for kw in ({}, {"weights": np.full((4, A), 1.0 / A)}, {"corr": C}, {"weights": np.full(A, 1.0 / A), "corr": C}):
        new = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, normalize=normalize, **kw)
        np.testing.assert_allclose(new.cols, old.cols, rtol=1e-12, atol=0.0)
        np.testing.assert_allclose(new.tot, old.tot, rtol=1e-12, atol=0.0)
        # not smaller, up to the f64 rounding of the two ways of writing the same expression
        assert np.all(new.cols_bound >= old.cols_bound * (1.0 - 1e-12))
        assert np.all(new.tot_bound >= old.tot_bound * (1.0 - 1e-12))
        np.testing.assert_array_equal(new.doubt, old.doubt)


@pytest.mark.parametrize("normalize", [True, False], ids=["NORMALIZE", "RAW"])
def test_margrabe_exchange_option(normalize) -> None:
    """A = 2, weights (1, -1), K = 0: column 1 is the exchange option, whose value is a closed form in rho."""
    rows = cases.margrabe_rows()
    m = cases.MARGRABE
    ref = gr.reference(_oracle, rows, 2, m["T"], m["P"], m["seed"], m["ordinal0"], weights=np.array([1.0, -1.0]),
                       normalize=normalize)
    want = gr.margrabe(rows)
    F1 = br.forwards(rows, 2)[0][:, 1]
    assert np.all(want >= 0.019 * F1)  # no contract whose value is lost in the noise
    z = np.abs(ref.cols[:, 1] - want) / ref.cols[:, 7]
    print(f"Margrabe, {'NORMALIZE' if normalize else 'RAW'}: worst {z.max():.2f} standard errors")
    assert np.all(z < 5.0), z
    # and the put side by parity: call - put = df (F_0 - F_1) in the mean of bk
    df = br.forwards(rows, 2)[2]
    np.testing.assert_allclose(ref.cols[:, 1] - ref.cols[:, 0], df * ref.cols[:, 12], rtol=1e-9, atol=1e-12)


def _misses(got: np.ndarray, ref: gr.GeneralRef, col: int) -> int:
    """Contracts whose column lies outside the bound (a non-finite value does)."""
    return int((~(np.abs(got[:, col] - ref.cols[:, col]) <= ref.cols_bound[:, col])).sum())


def _device_factor(C: np.ndarray) -> np.ndarray:
    """The factor a kernel would make of a matrix it misread: the header's statements, which go through (clamping a
    negative pivot to 0) where numpy.linalg.cholesky refuses an indefinite matrix."""
    A = C.shape[0]
    L = np.zeros((A, A))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(A):
            for k in range(i + 1):
                s = 1.0 if i == k else C[i, k]
                for m in range(k):
                    s = s - L[i, m] * L[k, m]
                L[i, k] = np.sqrt(s if s > 0.0 else 0.0) if i == k else np.float64(s) / L[k, k]
    return L


def test_packed_triangle_read_column_major_leaves_the_bound(case_4_16_4096) -> None:
    rows, w, C, ref = case_4_16_4096
    A, T, P, norm, B = cases.CASES[0]
    tri = cases.pack(C)  # row-major: (1,0), (2,0), (2,1), (3,0), (3,1), (3,2)
    wrong = np.stack([np.eye(A)] * B)
    order = [(i, k) for k in range(A) for i in range(k + 1, A)]  # column-major: (1,0), (2,0), (3,0), (2,1), ...
    for n, (i, k) in enumerate(order):
        wrong[:, i, k] = wrong[:, k, i] = tri[:, n]
    assert not np.array_equal(wrong, C)
    np.testing.assert_allclose(np.stack([_device_factor(c) for c in C]), gr.factors(rows, A, C), rtol=1e-12, atol=1e-14)
    Lw = np.stack([_device_factor(c) for c in wrong])
    with np.errstate(all="ignore"):
        bad = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, weights=w, L=Lw, normalize=bool(norm))
    assert _misses(bad.cols, ref, 0) >= B // 2, _misses(bad.cols, ref, 0)


def test_transposed_factor_leaves_the_bound(case_4_16_4096) -> None:
    rows, w, C, ref = case_4_16_4096
    A, T, P, norm, B = cases.CASES[0]
    Lt = np.ascontiguousarray(gr.factors(rows, A, C).transpose(0, 2, 1))
    bad = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, weights=w, L=Lt, normalize=bool(norm))
    assert _misses(bad.cols, ref, 0) >= B // 2, _misses(bad.cols, ref, 0)


def test_weights_applied_to_best_and_worst_leave_the_bound(case_4_16_4096) -> None:
    """The weights do not touch the basket column here, so this reading is looked for where it shows: the best-of and
    worst-of puts (columns 2 and 4) and the means of mx and mn (13, 14)."""
    rows, w, C, ref = case_4_16_4096
    A, T, P, norm, B = cases.CASES[0]
    wx = w[:, :, None] * ref.xs
    u = np.stack([ref.u[0], wx.max(axis=1), wx.min(axis=1)])
    bad, _, _ = gr.price_columns(rows, A, u, ref.du, w)
    np.testing.assert_array_equal(bad[:, 0], ref.cols[:, 0])
    for col in (2, 4, 13, 14):
        assert _misses(bad, ref, col) >= B // 2, (col, _misses(bad, ref, col))


def test_absolute_weights_on_a_spread_row_leave_the_bound() -> None:
    """(4, 16, 4096) with the signs (+, -, +, -) on the drawn weights; K follows sum w_i F_i where that is positive."""
    A, T, P, norm, B = cases.CASES[0]
    rows, w, C = cases.drawn_case(_oracle, A, B)
    ws = w * np.array([1.0, -1.0, 1.0, -1.0])
    F = br.forwards(rows, A)[0]
    rows[:, 0] = np.maximum((ws * F).sum(axis=1), 0.0)
    ref = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, weights=ws, corr=C, normalize=bool(norm))
    bad = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, weights=np.abs(ws), corr=C, normalize=bool(norm))
    assert _misses(bad.cols, ref, 0) >= B // 2, _misses(bad.cols, ref, 0)


def test_weighted_sum_bound_uses_absolute_values() -> None:
    """A spread whose legs cancel: the plain-sum form of the bound would be (nearly) zero, this one is not."""
    xs = np.array([[[100.0], [100.0]]])
    dxs = np.full_like(xs, 1e-5)
    w = np.array([[1.0, -1.0]])
    bk, dbk = gr.weighted(xs, dxs, w)
    assert bk[0, 0] == 0.0
    assert dbk[0, 0] >= 2e-5 + 3 * br.U * 200.0 * (1 - 1e-9)
    one, done = gr.weighted(xs, dxs, np.array([[0.5, 0.5]]))
    old, dold = br._mean_of(xs, dxs, 2)
    np.testing.assert_allclose(one, old, rtol=1e-15)
    np.testing.assert_allclose(done, dold, rtol=1e-12)
