"""tests/helpers/basket_path_reference.py on the CPU: its last row and its European and worst-of columns are the
weighted, general-correlation reference's; the barriers of every case the GPU test uses leave at most
max(2, P / 256) knocked flags per contract and barrier in doubt (a condition on the inputs, asserted here and before
the kernel's output is looked at there); and five wrong readings of the documented meaning leave its bound, which is
what gives tests/test_gpu_basket_path.py teeth (a CPU restatement of the kernel's f32 arithmetic is not kept)."""

from __future__ import annotations

import numpy as np
import pytest

import oracle as _oracle
from tests.helpers import basket_general_reference as gr
from tests.helpers import basket_path_cases as pc
from tests.helpers import basket_path_reference as pr
from tests.helpers import basket_reference as br

SEED, ORD0 = pc.SEED, pc.ORD0
ALL = [(c, False) for c in pc.CASES] + [(pc.SPREAD, True)]
IDS = [f"A{c[0]}-T{c[1]}-P{c[2]}" + ("-spread" if s else "") for c, s in ALL]


def _misses(cols: np.ndarray, ref: pr.PathRef, col: int) -> int:
    """Contracts whose column lies outside the bound (a non-finite value does)."""
    return int((~(np.abs(cols[:, col] - ref.cols[:, col]) <= ref.cols_bound[:, col])).sum())


@pytest.mark.parametrize("case,spread", ALL, ids=IDS)
def test_no_contract_of_any_case_is_dropped(case, spread) -> None:
    """The condition on the inputs: the default barriers are live (some paths knocked, not all) and leave few flags
    in doubt, in both math modes and under both normalisations."""
    A, T, P, B = case
    rows, w, _, bars = pc.inputs(_oracle, A, B, spread)
    assert np.all(bars[:, 0] < bars[:, 1]) and np.all(np.isfinite(bars))
    for math in pc.EPS:
        for normalize in (True, False):
            ref = pc.reference(_oracle, A, T, P, B, math, normalize, spread)
            assert pr.count_ok(ref.doubt[:, 0], P) and pr.count_ok(ref.doubt[:, 1], P), (math, normalize, ref.doubt)
            assert np.all(np.isfinite(ref.cols)) and np.all(np.isfinite(ref.cols_bound))
            assert np.all(ref.cols_bound >= 0.0)
    ref = pc.reference(_oracle, A, T, P, B, "portable", True, spread)
    print(f"{case}: knocked share {ref.cols[:, 21].round(3)}, worst {ref.cols[:, 22].round(3)}, doubt {ref.doubt.max(axis=0)}")
    assert 0.02 < ref.cols[:, 21].mean() < 0.98 and 0.0 < ref.cols[:, 22].mean() < 0.98


@pytest.mark.parametrize("normalize", [True, False], ids=["NORMALIZE", "RAW"])
def test_last_row_is_the_general_reference(normalize) -> None:
    """Columns 8, 9, 18, 19 and the terminal sums are basket_general_reference's 0, 1, 6, 7 and tot; without barriers
    the worst-of columns are its 4, 5, 10, 11 and the knock-out columns the European ones; at T = 1 the Asian and
    lookback columns are the European ones."""
    A, T, P, B = pc.CASES[1]
    rows, w, C, _ = pc.inputs(_oracle, A, B)
    old = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=normalize)
    new = pc.reference(_oracle, A, T, P, B, "portable", normalize, False, False)
    np.testing.assert_allclose(new.tot, old.tot, rtol=1e-13, atol=0.0)
    for mine, theirs in (([8, 9, 18, 19], [0, 1, 6, 7]), ([6, 7, 16, 17], [4, 5, 10, 11]), ([2, 3, 12, 13], [0, 1, 6, 7])):
        np.testing.assert_allclose(new.cols[:, mine], old.cols[:, theirs], rtol=1e-11, atol=1e-13)
        assert np.all(new.cols_bound[:, mine] >= old.cols_bound[:, theirs] * (1.0 - 1e-9))
    assert np.all(new.cols[:, 21:23] == 0.0) and np.all(new.doubt == 0)
    one = pr.reference(_oracle, rows, A, 1, P, SEED, ORD0, weights=w, corr=C, normalize=normalize)
    np.testing.assert_allclose(one.cols[:, [0, 1, 4, 5]], one.cols[:, [8, 9, 8, 9]], rtol=1e-13, atol=0.0)
    np.testing.assert_allclose(one.cols[:, [23, 24]], one.cols[:, [20, 20]], rtol=1e-13, atol=0.0)


def test_orderings_of_the_reference() -> None:
    for case, spread in ALL:
        A, T, P, B = case
        c = pc.reference(_oracle, A, T, P, B, "portable", True, spread).cols
        assert np.all(c[:, 2] <= c[:, 8]) and np.all(c[:, 3] <= c[:, 9]) and np.all(c[:, 4] >= c[:, 8])
        assert np.all(c[:, 5] >= c[:, 9]) and np.all(c[:, 24] <= c[:, 20]) and np.all(c[:, 20] <= c[:, 23])


# ---- wrong readings leave the bound --------------------------------------------------------------------------------
def _wrong(case, spread, normalize, **wrong) -> tuple[pr.PathRef, np.ndarray]:
    A, T, P, B = case
    rows, w, _, bars = pc.inputs(_oracle, A, B, spread)
    x, rel = pc.simulated(_oracle, A, T, P, B, "hw", spread)  # the wider of the two bounds
    return pc.reference(_oracle, A, T, P, B, "hw", normalize, spread), \
        pr.outputs(rows, A, x, rel, w, bars, normalize, **wrong).cols


@pytest.mark.parametrize("normalize", [True, False], ids=["NORMALIZE", "RAW"])
def test_x0_monitored_leaves_the_bound(normalize) -> None:
    for case in pc.CASES[:2]:
        ref, cols = _wrong(case, False, normalize, with_x0=True)
        for col in (20, 0, 24):  # the mean average, the Asian put, the mean minimum
            assert _misses(cols, ref, col) * 2 >= case[3], (case, col, _misses(cols, ref, col))


@pytest.mark.parametrize("normalize", [True, False], ids=["NORMALIZE", "RAW"])
def test_average_divided_by_t_plus_one_leaves_the_bound(normalize) -> None:
    for case in pc.CASES[:3]:
        ref, cols = _wrong(case, False, normalize, divide_by=case[1] + 1)
        for col in (20, 1):  # the mean average, the Asian call
            assert _misses(cols, ref, col) * 2 >= case[3], (case, col, _misses(cols, ref, col))
        assert _misses(cols, ref, 8) == 0 and _misses(cols, ref, 23) == 0  # nothing else moves


def test_terminal_scale_on_every_row_leaves_the_bound() -> None:
    for case in pc.CASES[:2]:
        ref, cols = _wrong(case, False, True, terminal_scale=True)
        for col in (20, 23):  # the mean average, the mean maximum
            assert _misses(cols, ref, col) * 2 >= case[3], (case, col, _misses(cols, ref, col))
        assert _misses(cols, ref, 8) == 0 and _misses(cols, ref, 9) == 0  # the last row has its own scale
    # under RAW there is no scale to misplace
    ref, cols = _wrong(pc.CASES[1], False, False, terminal_scale=True)
    np.testing.assert_array_equal(cols, ref.cols)


@pytest.mark.parametrize("normalize", [True, False], ids=["NORMALIZE", "RAW"])
def test_min_over_weighted_values_leaves_the_bound(normalize) -> None:
    for case in (pc.CASES[0], pc.CASES[2]):
        ref, cols = _wrong(case, False, normalize, weighted_min=True)
        for col in (6, 22):  # the worst-of put, the share knocked on the worst asset
            assert _misses(cols, ref, col) * 2 >= case[3], (case, col, _misses(cols, ref, col))
        assert _misses(cols, ref, 2) == 0 and _misses(cols, ref, 21) == 0  # the basket's flag does not see it


@pytest.mark.parametrize("normalize", [True, False], ids=["NORMALIZE", "RAW"])
def test_strict_comparisons_leave_the_bound_on_a_level_taken_exactly(normalize) -> None:
    """paths() never gives a level a zero bound, so a level "taken exactly" is made here: the case's levels with their
    bounds set to zero (an exact kernel; the levels rounded to f32 so that the barrier costs no rounding) and, per contract, the upper barrier on the largest level of all its paths
    and dates, the other barriers off.  <= and >= then knock that one path, < and > none: column 21 is 1 / P against
    0 with no flag in doubt, and the knock-out call loses or keeps that path's payoff."""
    A, T, P, B = pc.CASES[1]
    rows, w, _, _ = pc.inputs(_oracle, A, B)
    ref = pc.reference(_oracle, A, T, P, B, "portable", normalize)
    b = ref.b.astype(np.float32).astype(np.float64)  # levels and a barrier an f32 kernel can hold
    top = b.reshape(B, -1).max(axis=1)
    bars = np.stack([np.full(B, -np.inf), top, np.full(B, -np.inf)], axis=1)
    zero = np.zeros_like(b)
    m = np.ones_like(b)  # the worst level is not looked at (its barrier is off)
    right = pr.path_columns(rows, A, b, zero, m, zero, bars, w)
    wrong = pr.path_columns(rows, A, b, zero, m, zero, bars, w, strict=True)
    assert np.all(right[2] == 0) and np.all(right[1][:, 21] == 0.0)
    np.testing.assert_array_equal(right[0][:, 21], np.full(B, 1.0 / P))
    assert np.all(wrong[0][:, 21] == 0.0)
    assert int((np.abs(wrong[0][:, 21] - right[0][:, 21]) > right[1][:, 21]).sum()) * 2 >= B
    # the same barrier on the lower side, and with the case's real bounds the path is in doubt, not decided
    lows = np.stack([b.reshape(B, -1).min(axis=1), np.full(B, np.inf), np.full(B, -np.inf)], axis=1)
    assert np.all(pr.path_columns(rows, A, b, zero, m, zero, lows, w)[0][:, 21] == 1.0 / P)
    assert np.all(pr.path_columns(rows, A, b, zero, m, zero, lows, w, strict=True)[0][:, 21] == 0.0)
    real = pr.path_columns(rows, A, b, ref.db, m, zero, bars, w)
    assert np.all(real[2][:, 0] >= 1)
