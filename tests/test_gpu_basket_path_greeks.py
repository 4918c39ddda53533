"""basket_path_greeks_kernel (smc_basket_greeks_paths) on the device, every output into NaN-poisoned buffers: the
bit-for-bit relations the header states.  The price columns and their errors are smc_basket_price_paths' columns 0, 1,
4, 5 and 10, 11, 14, 15; the block is the same run to run, under a 3 + 3 split with ordinal0, with the ordinal on the
device, with stride 0 against the row materialised B times, with an all-rho table against no table, with and without
SMC_PRICE_REPLAY; the rows a one-sweep shape and a several-sweep shape share give the same values; small shapes are
finite and every standard error is exactly 0 at P = 1.  A = 1..8 all appear, in both maths and both normalisations.
The independent float64 reference is tests/test_gpu_basket_path_greeks_reference.py's."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from spectralmc_amd import _lib
from spectralmc_amd.basket import BasketConfig, basket_greeks_paths, basket_path_greeks_fields
from tests.helpers import assert_rows_equal, poisoned
from tests.helpers import basket_general_cases as cases
from tests.helpers import basket_path_greeks_cases as gc
from tests.helpers import basket_path_greeks_reference as pg

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, ORD0 = gc.SEED, gc.ORD0
MATHS = {"portable": 0, "hw": _lib.MATH_HW}
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE


def _dev(a: np.ndarray | None) -> torch.Tensor | None:
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _greeks(rows: np.ndarray, A: int, T: int, P: int, flags: int, norm: int, *, w: np.ndarray | None = None,
            ws: int | None = None, tri: np.ndarray | None = None, cs: int | None = None, ordinal0: int = ORD0,
            ordinal_dev: torch.Tensor | None = None, finite: bool = True) -> np.ndarray:
    """The block [B, 16A + 24] of one C call; w [A] or [B, A], tri [n] or [B, n] (strides default to 0 for a single
    row, to the row length otherwise)."""
    B = rows.shape[0]
    cd, wd, td = _dev(rows), _dev(w), _dev(tri)
    ws = (0 if w is None or w.ndim == 1 else w.shape[1]) if ws is None else ws
    cs = (0 if tri is None or tri.ndim == 1 else tri.shape[1]) if cs is None else cs
    out = poisoned((B, _lib.basket_path_greeks_cols(A)), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_greeks_paths(
        _lib.ptr(cd), _lib.ptr(wd), ws, _lib.ptr(td), cs, B, A, T, P, SEED, _lib.ptr(ordinal_dev), ordinal0, flags, norm,
        _lib.ptr(out), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    if finite:
        assert np.isfinite(got).all()
    return got


def _prices(rows: np.ndarray, A: int, T: int, P: int, flags: int, norm: int, w: np.ndarray, tri: np.ndarray | None) -> np.ndarray:
    B = rows.shape[0]
    cd, wd, td = _dev(rows), _dev(w), _dev(tri)
    out = poisoned((B, _lib.BASKET_PATH_COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price_paths(
        _lib.ptr(cd), _lib.ptr(wd), w.shape[1], _lib.ptr(td), 0 if tri is None else tri.shape[1], None, B, A, T, P, SEED,
        None, ORD0, flags, norm, _lib.ptr(out), None, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _case(A: int, B: int):
    rows, w, C = gc.inputs(A, B)
    return rows, w, (cases.pack(C) if A > 1 else None)


ALL = gc.CASES + [gc.SPREAD]


def test_every_asset_count_appears() -> None:
    assert {c[0] for c in ALL} == set(range(1, 9))


@pytest.mark.parametrize("case", ALL, ids=lambda c: f"A{c[0]}-T{c[1]}-P{c[2]}")
def test_price_columns_are_the_price_call(case) -> None:
    A, T, P, B = case
    rows, w, tri = _case(A, B)
    for hw in MATHS.values():
        for norm, label in ((NORM, b"replay"), (RAW, b"raw")):
            assert _lib.lib().smc_basket_greeks_paths_kernel(A, T, P, hw, norm) == \
                b"basket_path_greeks_kernel(" + label + b")"
            price = _prices(rows, A, T, P, hw, norm, w, tri)
            got = _greeks(rows, A, T, P, hw, norm, w=w, tri=tri)
            assert_rows_equal(got[:, pg.price_columns(A)], price[:, [0, 1, 4, 5, 10, 11, 14, 15]],
                              f"price columns A {A} T {T} P {P} math {hw} norm {norm}")


@pytest.mark.parametrize("case", [(4, 6, 693, 6), (5, 4, 2048, 6), (8, 3, 2048, 6), (1, 7, 2049, 6)],
                         ids=lambda c: f"A{c[0]}-T{c[1]}-P{c[2]}")
def test_block_is_the_same_run_to_run_split_ordinal_and_replay(case) -> None:
    A, T, P, B = case
    rows, w, tri = _case(A, B)
    for hw in MATHS.values():
        for norm in (NORM, RAW):
            base = _greeks(rows, A, T, P, hw, norm, w=w, tri=tri)
            assert_rows_equal(_greeks(rows, A, T, P, hw, norm, w=w, tri=tri), base, "run to run")
            halves = [_greeks(rows[s], A, T, P, hw, norm, w=w[s], tri=None if tri is None else tri[s],
                              ordinal0=ORD0 + s.start) for s in (slice(0, 3), slice(3, 6))]
            assert_rows_equal(np.concatenate(halves), base, "3 + 3 split")
            od = torch.tensor([ORD0 - 2], dtype=torch.int64, device=DEV)
            assert_rows_equal(_greeks(rows, A, T, P, hw, norm, w=w, tri=tri, ordinal0=2, ordinal_dev=od), base,
                              "ordinal on the device")
            assert_rows_equal(_greeks(rows, A, T, P, hw | _lib.PRICE_REPLAY, norm, w=w, tri=tri), base,
                              "SMC_PRICE_REPLAY")


@pytest.mark.parametrize("A", [3, 6])
def test_stride_zero_and_all_rho_table(A) -> None:
    T, P, B = 4, 693, 4
    rows, w, tri = _case(A, B)
    for hw in MATHS.values():
        for norm in (NORM, RAW):
            shared = _greeks(rows, A, T, P, hw, norm, w=w[0], tri=tri[0])
            tiled = _greeks(rows, A, T, P, hw, norm, w=np.tile(w[0], (B, 1)), tri=np.tile(tri[0], (B, 1)))
            assert_rows_equal(shared, tiled, "stride 0 is the row materialised B times")
            rows_rho = rows.copy()
            rows_rho[:, 3] = 0.3
            n = A * (A - 1) // 2
            with_table = _greeks(rows_rho, A, T, P, hw, norm, w=w, tri=np.full((B, n), 0.3))
            assert_rows_equal(with_table, _greeks(rows_rho, A, T, P, hw, norm, w=w), "an all-rho table is no table")
            none_w = _greeks(rows, A, T, P, hw, norm, tri=tri)
            assert none_w.shape == shared.shape  # weights NULL: 1 / A


@pytest.mark.parametrize("A,T_one,T_many", [(4, 4, 8), (8, 2, 4)])
def test_rows_shared_by_one_sweep_and_several_sweeps(A, T_one, T_many) -> None:
    """T_one dates are served by one NORMALIZE sweep of this kernel, T_many by two, while smc_basket_price_paths (half
    the accumulator rows per date) covers both in one.  The row sums are not an output, so the plan allows the
    comparison through the scales only: the prices, which read every row's scale, match the price call's bit for bit
    in both shapes, so a sweep boundary changes no row sum."""
    P, B = 2049, 3
    rows, w, tri = _case(A, B)
    for hw in MATHS.values():
        for T in (T_one, T_many):
            got = _greeks(rows, A, T, P, hw, NORM, w=w, tri=tri)
            price = _prices(rows, A, T, P, hw, NORM, w, tri)
            assert_rows_equal(got[:, pg.price_columns(A)], price[:, [0, 1, 4, 5, 10, 11, 14, 15]], f"T {T}")


@pytest.mark.parametrize("P", [1, 3, 2049])
def test_small_shapes_are_finite_and_one_path_has_no_error(P) -> None:
    A, T, B = 1, 1, 4
    rows, w, _ = _case(A, B)
    for hw in MATHS.values():
        for norm in (NORM, RAW):
            got = _greeks(rows, A, T, P, hw, norm, w=w)
            G = pg.kinds(A)
            if P == 1:
                assert np.all(got[:, 4 * G:8 * G] == 0.0) and np.all(got[:, 8 * G + 4:] == 0.0)
    for A in (4, 7):
        rows, w, tri = _case(A, B)
        got = _greeks(rows, A, 3, 1, 0, NORM, w=w, tri=tri)
        G = pg.kinds(A)
        assert np.all(got[:, 4 * G:8 * G] == 0.0) and np.all(got[:, 8 * G + 4:] == 0.0)


def test_python_surface_matches_the_c_call() -> None:
    A, T, P, B = 3, 5, 2048, 6
    rows, w, C = gc.inputs(A, B)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=32, mc_seed=SEED, normalize=True,
                       math="portable")
    res = basket_greeks_paths(_dev(rows), cfg, weights=_dev(w), correlation=_dev(C), ordinal0=ORD0, n_paths=P)
    torch.cuda.synchronize()
    want = _greeks(rows, A, T, P, 0, NORM, w=w, tri=cases.pack(C))
    assert_rows_equal(res.block.cpu().numpy(), want, "basket_greeks_paths")
    names = basket_path_greeks_fields(A)
    assert torch.equal(res.delta_lookback_call[:, 2], res.block[:, names.index("delta_lookback_call_2")])
    assert torch.equal(res.theta_asian_put, res.block[:, names.index("theta_asian_put")])
