"""Greeks of the weighted, general-correlation basket (smc_basket_greeks_general / basket_greeks(weights=,
correlation=) / BasketEngine.greeks): the [B][2 A^2 + 6 A + 12] block and the [B][A + A (A + 1) / 2] pass-1 sums of
basket_greeks_general_kernel.

Within a measured share of each column's standard error against the independent float64 reference
(tests/helpers/basket_general_greeks_reference.py), in both maths and in the raw, lds and forced-replay modes; bit for
bit where the header promises it (the prices and terminal sums against smc_basket_price_general, lds against replay,
run to run, under a split of the batch, the ordinal on the host or on the device, stride 0 against materialised rows,
an all-rho table against none, the delta, vega, rho and theta columns against smc_basket_greeks at A in {1, 2, 4, 8});
the pair columns against smc_basket_greeks's correlation column; Margrabe's closed form; the conventions; the Python
surface; a replayed graph.  Smallest shapes that reach every path: B = 3..6, T in {1, 3, 16}, A in {1, 2, 3, 5, 8},
P in {1, 5, 2047, 2049} and one P on each side of the parking bound at A = 8; the reference cases also hold every
other (A, normalisation) at T = 3, P = 693, so that every instantiation is compared (tests/test_instantiation_ledger.py)."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.basket import (BasketConfig, BasketEngine, BasketGeneralGreeks, BasketGreeks, basket_greeks,
                                   pack_correlation, unpack_correlation)
from tests.helpers import assert_rows_equal, poisoned
from tests.helpers import basket_general_cases as gcases
from tests.helpers import basket_general_greeks_cases as cases
from tests.helpers import basket_general_greeks_reference as gg
from tests.helpers import basket_greeks_cases as eq_cases
from tests.helpers import basket_reference as br
from tests.helpers import instantiations as inst

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, ORD0 = cases.SEED, cases.ORD0
HW, REPLAY = _lib.MATH_HW, _lib.PRICE_REPLAY
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
# The share of a column's own standard error the device may lie from the float64 reference: 4 times the largest
# departure of the float32 restatement on the CPU (measured 2.34e-5, held to MEASURED_SHARE = 2.5e-5 by
# tests/test_basket_general_greeks_reference.py), so 1.0e-4.  Largest share seen on the MI355X: 2.70e-5 (hw math,
# A = 8, T = 1, P = 4109, replay); portable math gave the CPU's 2.34e-5.
ALLOWED = cases.ALLOWED_SHARE


def _dev(a: np.ndarray | None) -> torch.Tensor | None:
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _greeks(c, A, T, P, math_, norm, *, w=None, ws=None, tri=None, cs=None, ordinal0=ORD0, ordinal_dev=None):
    """(block, sums) of one smc_basket_greeks_general call into NaN-poisoned outputs.  w [A] or [B, A], tri packed rows
    [np] or [B, np] (numpy); the strides default to 0 for one row and the row length otherwise."""
    B = c.shape[0]
    cd, wd, td = _dev(c), _dev(w), _dev(tri)
    if tri is not None and tri.size == 0:
        td = None
    ws = (0 if w is None or w.ndim == 1 else w.shape[1]) if ws is None else ws
    cs = (0 if tri is None or tri.ndim == 1 else tri.shape[1]) if cs is None else cs
    out = poisoned((B, 2 * A * A + 6 * A + 12), torch.float64, DEV)
    sums = poisoned((B, A + A * (A + 1) // 2), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_greeks_general(_lib.ptr(cd), _lib.ptr(wd), ws, _lib.ptr(td), cs, B, A, T, P, SEED,
                                                    _lib.ptr(ordinal_dev), ordinal0, math_, norm, _lib.ptr(out),
                                                    _lib.ptr(sums), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), sums.cpu().numpy()


def _price_general(c, A, T, P, math_, norm, w, tri):
    B = c.shape[0]
    cd, wd, td = _dev(c), _dev(w), _dev(tri)
    if tri is not None and tri.size == 0:
        td = None
    out = poisoned((B, _lib.BASKET_PRICE_COLS), torch.float64, DEV)
    tsum = poisoned((B, A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price_general(
        _lib.ptr(cd), _lib.ptr(wd), 0 if w is None or w.ndim == 1 else A, _lib.ptr(td),
        0 if tri is None or tri.ndim == 1 else tri.shape[1], B, A, T, P, SEED, None, ORD0, math_, norm, _lib.ptr(out),
        _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tsum.cpu().numpy()


def _greeks_equal_weight(c, A, T, P, math_, norm):
    out = poisoned((c.shape[0], 8 * A + 16), torch.float64, DEV)
    sums = poisoned((c.shape[0], 3, A), torch.float64, DEV)
    cd = _dev(c)
    _lib.check(_lib.lib().smc_basket_greeks(_lib.ptr(cd), c.shape[0], A, T, P, SEED, None, ORD0, math_, norm,
                                            _lib.ptr(out), _lib.ptr(sums), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), sums.cpu().numpy()


def _name(A, T, P, math_, norm) -> str:
    return _lib.lib().smc_basket_greeks_general_kernel(A, T, P, math_, norm).decode()


@functools.lru_cache(maxsize=None)
def _reference(kind: str, A: int, T: int, P: int, norm: int, B: int) -> np.ndarray:
    """The float64 block of a reference case: computed once, shared, read-only."""
    _oracle.build()
    rows, w, C = cases.inputs(kind, A, B)
    ref, _ = gg.greeks(_oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=bool(norm))
    ref.setflags(write=False)
    return ref


def _n(A: int) -> int:
    return cases.greek_columns(A)


# --------------------------------------------------------------------------- 1. the float64 reference
@pytest.mark.parametrize("kind,A,T,P,norm,B", cases.REFERENCE_CASES)
def test_every_column_within_the_allowed_share_of_the_reference(kind, A, T, P, norm, B) -> None:
    """Both maths; the mode the shape selects (raw under RAW, lds or replay by the parking bound) and forced replay."""
    rows, w, C = cases.inputs(kind, A, B)
    tri = gcases.pack(C)
    ref = _reference(kind, A, T, P, norm, B)
    want_mode = "raw" if not norm else ("replay" if (A, P) == (8, cases.PARK_FIRST_REPLAY) else "lds")
    assert _name(A, T, P, 0, norm) == f"basket_greeks_general_kernel({want_mode})"
    worst = {}
    # every launch the ledger counts for the row (raw has no second mode, and the replay case runs replay by itself)
    runs = inst.pricing_runs_of("basket general greeks", (kind, A, T, P, norm, B))
    assert len(runs) == (4 if want_mode == "lds" else 2) and all(r.normalize == bool(norm) for r in runs)
    for run in runs:
        math_ = (HW if run.math == "hw" else 0) | (REPLAY if run.force_replay else 0)
        assert _name(A, T, P, math_, norm) == run.name
        got, _ = _greeks(rows, A, T, P, math_, norm, w=w, tri=tri)
        assert got.shape == ref.shape and not np.isnan(got).any()
        shares = cases.shares_of_stderr(got, ref, rows, A)
        col = max(shares, key=shares.get)
        print(f"{kind} A {A} T {T} P {P} norm {norm} math {math_:#x}: largest share of a standard error "
              f"{shares[col]:.3e} (column {col}); allowed {ALLOWED:.1e}")
        worst[math_] = (shares[col], col)
        # the standard errors themselves: the reference's, to float32 accuracy of the terms
        n = _n(A)
        se = list(range(n, 2 * n)) + [2 * n + 2, 2 * n + 3]
        means = list(range(n)) + [2 * n, 2 * n + 1]
        assert np.all(np.abs(got[:, se] - ref[:, se]) <= 2e-4 * ref[:, se] + 1e-7 * np.abs(ref[:, means])), "standard errors"
    assert all(v[0] <= ALLOWED for v in worst.values()), worst


# --------------------------------------------------------------------------- 2. bit for bit
BIT_CASES = [(1, 3, 5, NORM, 3), (2, 1, 2049, NORM, 4), (3, 16, 2047, NORM, 3), (5, 3, 2049, RAW, 3), (5, 3, 2047, NORM, 3),
             (8, 1, 1, NORM, 3), (8, 3, cases.PARK_LAST, NORM, 3), (8, 1, cases.PARK_FIRST_REPLAY, NORM, 3)]


@pytest.mark.parametrize("A,T,P,norm,B", BIT_CASES)
def test_prices_and_terminal_sums_are_the_price_calls(A, T, P, norm, B) -> None:
    """(a): columns 2n .. 2n + 3 and tot against smc_basket_price_general's columns 0, 1, 6, 7 and terminal_sum_dev."""
    rows, w, C = cases.inputs("drawn", A, B)
    tri = gcases.pack(C)
    n = _n(A)
    for math_ in (0, HW):
        got, sums = _greeks(rows, A, T, P, math_, norm, w=w, tri=tri)
        price, tsum = _price_general(rows, A, T, P, math_, norm, w, tri)
        assert_rows_equal(got[:, 2 * n:2 * n + 4], price[:, [0, 1, 6, 7]], "prices")
        assert_rows_equal(sums[:, :A], tsum, "terminal sums")
        if norm == RAW:
            assert np.all(sums[:, A:] == 0.0)
        else:
            assert not np.isnan(sums).any()
        if P == 1:
            assert np.all(got[:, n:2 * n] == 0.0) and np.all(got[:, 2 * n + 2:] == 0.0)


@pytest.mark.parametrize("A,T,P,norm,B", BIT_CASES)
def test_lds_is_replay_run_to_run_split_and_device_ordinal(A, T, P, norm, B) -> None:
    """(b): the whole block and the sums, A = 8 with all its passes included."""
    rows, w, C = cases.inputs("drawn", A, B)
    tri = gcases.pack(C)
    for math_ in (0, HW):
        base = _greeks(rows, A, T, P, math_, norm, w=w, tri=tri)
        for what, other in (
                ("replay", _greeks(rows, A, T, P, math_ | REPLAY, norm, w=w, tri=tri)),
                ("again", _greeks(rows, A, T, P, math_, norm, w=w, tri=tri)),
                ("device ordinal", _greeks(rows, A, T, P, math_, norm, w=w, tri=tri, ordinal0=1,
                                           ordinal_dev=torch.tensor([ORD0 - 1], dtype=torch.int64, device=DEV)))):
            assert_rows_equal(other[0], base[0], what)
            assert_rows_equal(other[1], base[1], what + " sums")
        head = _greeks(rows[:1], A, T, P, math_, norm, w=w[:1], tri=tri[:1])
        tail = _greeks(rows[1:], A, T, P, math_, norm, w=w[1:], tri=tri[1:], ordinal0=ORD0 + 1)
        assert_rows_equal(np.concatenate([head[0], tail[0]]), base[0], "split")
        assert_rows_equal(np.concatenate([head[1], tail[1]]), base[1], "split sums")


@pytest.mark.parametrize("A,T,P,norm,B", [(3, 3, 2049, NORM, 4), (5, 1, 5, RAW, 3), (8, 1, 2047, NORM, 3)])
def test_shared_rows_and_the_all_rho_table(A, T, P, norm, B) -> None:
    """(c) stride 0 is the row materialised B times (also with padded strides); (d) an all-rho table is no table."""
    rows, w, C = cases.inputs("drawn", A, B)
    tri = gcases.pack(C)
    npr = tri.shape[1]
    for math_ in (0, HW):
        shared = _greeks(rows, A, T, P, math_, norm, w=w[0].copy(), tri=tri[0].copy())
        tiled = _greeks(rows, A, T, P, math_, norm, w=np.tile(w[0], (B, 1)), tri=np.tile(tri[0], (B, 1)))
        assert_rows_equal(shared[0], tiled[0], "stride 0")
        assert_rows_equal(shared[1], tiled[1], "stride 0 sums")
        wp, tp = np.full((B, A + 3), np.nan), np.full((B, npr + 5), np.nan)
        wp[:, :A], tp[:, :npr] = w, tri
        padded = _greeks(rows, A, T, P, math_, norm, w=wp, tri=tp)
        assert_rows_equal(padded[0], _greeks(rows, A, T, P, math_, norm, w=w, tri=tri)[0], "padded strides")
        rho_tri = np.repeat(rows[:, 3:4], npr, axis=1)
        assert_rows_equal(_greeks(rows, A, T, P, math_, norm, w=w, tri=rho_tri)[0],
                          _greeks(rows, A, T, P, math_, norm, w=w)[0], "all-rho table")


@pytest.mark.parametrize("A,T,P,norm", [(1, 3, 2047, NORM), (2, 16, 2049, NORM), (4, 3, 2049, RAW), (4, 3, 2047, NORM),
                                         (8, 1, 2049, RAW), (8, 3, 2047, NORM)])
def test_equal_weights_and_equicorrelation_are_smc_basket_greeks(A, T, P, norm) -> None:
    """(e): with no tables, or explicit 1 / A and all-rho, the delta, vega, rho and theta columns and their errors and
    the prices are smc_basket_greeks's bit for bit (f32(1 / A) is a power of two); tot and sxl too; and the pair
    columns sum to its correlation column within the sum of their allowances."""
    B = 4
    rows = eq_cases.contracts(A, B)
    npr = A * (A - 1) // 2
    n, m = _n(A), 4 * A + 6
    for math_ in (0, HW):
        old, old_sums = _greeks_equal_weight(rows, A, T, P, math_, norm)
        for what, kw in (("no tables", {}), ("explicit", dict(w=np.full(A, 1.0 / A), tri=np.repeat(rows[:, 3:4], npr, axis=1)))):
            got, sums = _greeks(rows, A, T, P, math_, norm, **kw)
            assert_rows_equal(got[:, :4 * A + 4], old[:, :4 * A + 4], what)
            assert_rows_equal(got[:, n:n + 4 * A + 4], old[:, m:m + 4 * A + 4], what + " errors")
            assert_rows_equal(got[:, 2 * n:], old[:, 2 * m:], what + " prices")
            assert_rows_equal(sums[:, :A], old_sums[:, 0], what + " tot")
            diag = [A + i * (i + 1) // 2 + i for i in range(A)]
            assert_rows_equal(sums[:, diag], old_sums[:, 1], what + " sxl")
            for side in range(2):
                pair = got[:, 4 * A + 4 + side * npr:4 * A + 4 + (side + 1) * npr]
                err = got[:, n + 4 * A + 4 + side * npr:n + 4 * A + 4 + (side + 1) * npr]
                tol = ALLOWED * (err.sum(axis=1) + old[:, m + 4 * A + 4 + side])
                diff = np.abs(pair.sum(axis=1) - old[:, 4 * A + 4 + side])
                print(f"A {A} math {math_:#x} {what} side {side}: pair sum against the correlation column, largest share "
                      f"of the allowance {np.max(np.where(diff == 0, 0.0, diff / np.where(tol == 0, 1.0, tol))):.3e}")
                assert np.all(diff <= tol), (what, side)


# --------------------------------------------------------------------------- 3. closed form and conventions
def test_margrabe_deltas_and_correlation_sensitivity() -> None:
    """The 32 exchange options under RAW: both deltas and dV / drho = -X_1 e^{-d_1 T} phi(d_1) sqrt(T) v_1 v_2 / sigma
    within 5 of the device's own standard errors (the price test's multiple)."""
    rows = gcases.margrabe_rows()
    T, P = gcases.MARGRABE["T"], gcases.MARGRABE["P"]
    _, Tm, r, rho, X0, d, v = br.fields(rows, 2)
    sig = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2 - 2.0 * rho * v[:, 0] * v[:, 1])
    F = X0 * np.exp((r[:, None] - d) * Tm[:, None])
    d1 = (np.log(F[:, 0] / F[:, 1]) + 0.5 * sig * sig * Tm) / (sig * np.sqrt(Tm))
    Phi = lambda a: 0.5 * (1.0 + np.array([math.erf(t / math.sqrt(2.0)) for t in a]))  # noqa: E731
    want = np.stack([np.exp(-d[:, 0] * Tm) * Phi(d1), -np.exp(-d[:, 1] * Tm) * Phi(d1 - sig * np.sqrt(Tm)),
                     -X0[:, 0] * np.exp(-d[:, 0] * Tm) * np.exp(-0.5 * d1 * d1) / np.sqrt(2.0 * np.pi) * np.sqrt(Tm)
                     * v[:, 0] * v[:, 1] / sig], axis=1)
    n = _n(2)
    cols = [2, 3, 13]  # delta call 0, delta call 1, the pair's call column (4A + 4 + np = 13)
    for math_ in (0, HW):
        got, _ = _greeks(rows, 2, T, P, math_, RAW, w=np.array([1.0, -1.0]))
        z = np.abs(got[:, cols] - want) / got[:, [c + n for c in cols]]
        print(f"math {math_:#x}: worst |device - Margrabe| / stderr (delta 0, delta 1, correlation) {np.round(z.max(axis=0), 2).tolist()}")
        assert np.all(z <= 5.0), np.argwhere(z > 5.0).tolist()


def test_zero_volatility_and_zero_weight() -> None:
    A, T, P, B = 3, 3, 2049, 4
    rows, w, C = cases.inputs("drawn", A, B)
    tri = gcases.pack(C)
    n = _n(A)
    dead = rows.copy()
    dead[1, 4 + 2 * A + 2] = 0.0
    w0 = w.copy()
    w0[:, 1] = 0.0
    for math_ in (0, HW):
        for norm in (RAW, NORM):
            got, _ = _greeks(dead, A, T, P, math_, norm, w=w, tri=tri)
            pair = list(range(4 * A + 4, n)) + list(range(n + 4 * A + 4, 2 * n))
            rest = [c for c in range(2 * n + 4) if c not in pair]
            assert np.isnan(got[1, pair]).all() and not np.isnan(got[1, rest]).any()
            assert not np.isnan(np.delete(got, 1, axis=0)).any()
            for col in (2 * A + 2, 3 * A + 2):  # the vega of the deterministic asset and its error
                assert got[1, col] == 0.0 and got[1, n + col] == 0.0
            got, _ = _greeks(rows, A, T, P, math_, norm, w=w0, tri=tri)
            for col in (1, A + 1, 2 * A + 1, 3 * A + 1):  # delta and vega of the asset with weight 0
                assert np.all(got[:, col] == 0.0) and np.all(got[:, n + col] == 0.0)
            assert not np.isnan(got).any()


# --------------------------------------------------------------------------- 4. the Python surface and a graph
def test_python_surface_and_engine() -> None:
    A, T, P, B = 3, 3, 2049, 4
    rows, w, C = cases.inputs("drawn", A, B)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=32, mc_seed=SEED, normalize=True,
                       math="portable")
    cd, wd, Cd = _dev(rows), _dev(w), _dev(C)
    want, want_sums = _greeks(rows, A, T, P, 0, NORM, w=w, tri=gcases.pack(C))
    got = basket_greeks(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=Cd, validate=True)
    assert isinstance(got, BasketGeneralGreeks)
    assert_rows_equal(got.block.cpu().numpy(), want, "block")
    assert_rows_equal(torch.cat([got.terminal_sum, got.sum_moments], dim=1).cpu().numpy(), want_sums, "sums")
    packed = basket_greeks(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=pack_correlation(Cd), replay=True)
    assert_rows_equal(packed.block.cpu().numpy(), want, "packed rows, replay")
    n = _n(A)
    assert got.correlation_call.shape == (B, 3) and got.delta_put.shape == (B, A) and got.put.shape == (B,)
    assert torch.equal(got.correlation_put, got.block[:, 4 * A + 4:4 * A + 7])
    assert torch.equal(got.correlation_call_stderr, got.block[:, n + 4 * A + 7:2 * n])
    full = unpack_correlation(got.correlation_call, A)
    assert full.shape == (B, A, A) and torch.equal(full[:, 2, 1], got.block[:, 4 * A + 4 + 3 + 2])
    with pytest.raises(ValueError, match="positive definite"):
        basket_greeks(cd, cfg, n_paths=P, correlation=_dev(np.where(np.eye(A) == 1.0, 1.0, -0.9)), validate=True)
    # without the new arguments: smc_basket_greeks, unchanged
    plain = basket_greeks(cd, cfg, ordinal0=ORD0, n_paths=P)
    assert isinstance(plain, BasketGreeks)
    assert_rows_equal(plain.block.cpu().numpy(), _greeks_equal_weight(rows, A, T, P, 0, NORM)[0], "plain")
    engine = BasketEngine(cfg, B, device=torch.device(DEV), store_paths=False)
    eg = engine.greeks(cd, ordinal0=ORD0, n_paths=P, weights=wd, correlation=Cd)
    assert isinstance(eg, BasketGeneralGreeks)
    assert_rows_equal(eg.block.cpu().numpy(), want, "engine")
    assert isinstance(engine.greeks(cd, ordinal0=ORD0, n_paths=P), BasketGreeks)


def test_graph_capture_and_replay() -> None:
    A, T, P, B = 5, 3, 2049, 3
    rows, w, C = cases.inputs("drawn", A, B)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=32, mc_seed=SEED, normalize=True,
                       math="hw")
    cd, wd, td = _dev(rows), _dev(w), _dev(gcases.pack(C))
    want, _ = _greeks(rows, A, T, P, HW, NORM, w=w, tri=gcases.pack(C))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        basket_greeks(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=td)  # warm-up: the LDS attribute
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = basket_greeks(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=td)
    got.block.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(got.block.cpu().numpy(), want, "replayed graph")
