"""basket_path_greeks_kernel (smc_basket_greeks_paths) within the a-priori bound of the independent float64 reference
(tests/helpers/basket_path_greeks_reference.py): portable and SMC_MATH_HW math, RAW and NORMALIZE, A = 1..8, the
spread case included.  The reference, its bound and the two caps on the inputs (gbm_reference.count_ok on the
indicators in doubt, path_greeks_reference.arg_ok on the rows of an extreme in doubt) are computed and asserted before
the kernel's output is looked at; tests/test_basket_path_greeks_reference.py asserts the caps on the CPU and shows
that wrong readings leave the bound.

Largest share of the bound used on one MI355X: 0.114 for a Greek (A = 8, T = 3, P = 2048, portable, RAW), 0.053 for a
Greek's standard error, 0.043 for a price column."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from tests.helpers import basket_general_cases as cases
from tests.helpers import basket_general_greeks_cases as ggc
from tests.helpers import basket_general_greeks_reference as gg
from tests.helpers import basket_greeks_cases as eq_cases
from tests.helpers import basket_path_greeks_cases as gc
from tests.helpers import basket_path_greeks_reference as pg
from tests.helpers import basket_reference as br
from tests.helpers import instantiations as inst
from tests.helpers import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, ORD0 = gc.SEED, gc.ORD0
MATHS = {"portable": 0, "hw": _lib.MATH_HW}
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE


def _dev(a: np.ndarray | None) -> torch.Tensor | None:
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _greeks(rows, A, T, P, flags, norm, w, tri) -> np.ndarray:
    B = rows.shape[0]
    cd, wd, td = _dev(rows), _dev(w), _dev(tri)
    out = poisoned((B, _lib.basket_path_greeks_cols(A)), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_greeks_paths(
        _lib.ptr(cd), _lib.ptr(wd), w.shape[1], _lib.ptr(td), 0 if tri is None else tri.shape[1], B, A, T, P, SEED,
        None, ORD0, flags, norm, _lib.ptr(out), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


def _general(rows, A, T, P, flags, norm, w, tri) -> np.ndarray:
    B = rows.shape[0]
    cd, wd, td = _dev(rows), _dev(w), _dev(tri)
    out = poisoned((B, _lib.basket_greeks_general_cols(A)), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_greeks_general(
        _lib.ptr(cd), _lib.ptr(wd), w.shape[1], _lib.ptr(td), 0 if tri is None else tri.shape[1], B, A, T, P, SEED,
        None, ORD0, flags, norm, _lib.ptr(out), None, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _against_reference(case, spread: bool) -> None:
    A, T, P, B = case
    _oracle.build()
    rows, w, C = gc.inputs(A, B, spread)
    tri = cases.pack(C) if A > 1 else None
    # every launch the ledger counts for the row: both maths, NORMALIZE and RAW
    for run in inst.pricing_runs_of("basket path greeks", case):
        math, hw, norm = run.math, MATHS[run.math], (NORM if run.normalize else RAW)
        assert _lib.lib().smc_basket_greeks_paths_kernel(A, T, P, hw, norm).decode() == run.name
        ref = gc.reference(_oracle, A, T, P, B, math, bool(norm), spread)
        # the conditions on the inputs, before the kernel's output is looked at
        assert pg.count_ok(ref.doubt_ind, P), ref.doubt_ind
        assert pg.arg_ok(ref.doubt_arg, P), ref.doubt_arg
        assert np.all(np.isfinite(ref.bound))
        got = _greeks(rows, A, T, P, hw, norm, w, tri)
        G = pg.kinds(A)
        used = {"greeks": pg.share_used(got, ref, list(range(4 * G))),
                "greek errors": pg.share_used(got, ref, list(range(4 * G, 8 * G))),
                "prices": pg.share_used(got, ref, pg.price_columns(A))}
        print(f"basket path greeks A {A} T {T} P {P} {math} {'NORMALIZE' if norm else 'RAW'}: share of the bound "
              "used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
        assert max(used.values()) < 1.0, (case, math, norm, used)


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: f"A{c[0]}-T{c[1]}-P{c[2]}")
def test_every_column_within_the_reference_bound(case) -> None:
    _against_reference(case, False)


def test_spread_within_the_reference_bound() -> None:
    """A = 2, weights (1, -0.5): a negative weight flips the signs of that asset's delta and vega by itself."""
    rows, w, _ = gc.inputs(2, gc.SPREAD[3], True)
    assert np.all(w[:, 1] < 0.0)
    _against_reference(gc.SPREAD, True)


@pytest.mark.parametrize("A,P", [(1, 2048), (3, 693), (4, 2049), (8, 1000)])
def test_one_time_step_is_the_european_greeks(A, P) -> None:
    """T = 1: the average, the maximum and the minimum of b_t are the terminal basket level, so delta_i, vega_i, rho
    and theta of the Asian and of the lookback pair are smc_basket_greeks_general's columns: each kernel within its
    own reference's tolerance of the one model value (this kernel's a-priori bound; that kernel's allowed share of its
    reference's standard error, the rho columns first giving up the constant's bound, as its own test states it)."""
    _oracle.build()
    B, T = 4, 1
    rows, w, C = gc.inputs(A, B)
    tri = cases.pack(C) if A > 1 else None
    n = gg.greek_columns(A)
    for math, hw in MATHS.items():
        for norm in (NORM, RAW):
            ref = gc.reference(_oracle, A, T, P, B, math, bool(norm))
            assert pg.count_ok(ref.doubt_ind, P) and pg.arg_ok(ref.doubt_arg, P)
            eref, _ = gg.greeks(_oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=bool(norm))
            got = _greeks(rows, A, T, P, hw, norm, w, tri)
            eur = _general(rows, A, T, P, hw, norm, w, tri)
            const = eq_cases.rho_constant_bound(rows, A)
            for g in range(pg.kinds(A)):
                for q in range(4):
                    a = pg.column(A, g, q)
                    side = q & 1
                    if g < 2 * A:
                        e = (2 * (g // A) + side) * A + g % A     # delta_put_i, delta_call_i, vega_put_i, vega_call_i
                    else:
                        e = 4 * A + 2 * (g - 2 * A) + side        # rho_put, rho_call, theta_put, theta_call
                    model = np.abs(ref.cols[:, a] - eref[:, e])   # the two references state one model
                    assert np.all(model <= 1e-11 * (1.0 + np.abs(eref[:, e]))), (g, q, model)
                    tol = ref.bound[:, a] + ggc.ALLOWED_SHARE * eref[:, n + e] + model
                    if g == 2 * A:
                        tol = tol + const
                    assert np.all(np.abs(got[:, a] - eur[:, e]) <= tol), (A, math, norm, g, q)


def test_flat_contract_is_held_on_delta_and_rho() -> None:
    """Every v_i = 0 and r = d_i: every row stays on X0_i exactly, the rows tie, the first row wins.  Delta and rho
    (and the prices) are held to the reference's bound; vega is exactly 0."""
    _oracle.build()
    A, T, P = 3, 4, 693
    rows, w, C = gc.flat_inputs(A)
    z, rad = pg.draws(_oracle, rows, A, T, P, SEED, ORD0)
    for math, hw in MATHS.items():
        for norm in (NORM, RAW):
            ref = pg.greeks(rows, A, T, z, rad, w, np.linalg.cholesky(C), math, normalize=bool(norm))
            assert np.all(ref.doubt_arg == 0)
            got = _greeks(rows, A, T, P, hw, norm, w, cases.pack(C))
            held = [pg.column(A, g, q) for g in list(range(A)) + [2 * A, pg.kinds(A)] for q in range(4)]
            assert br.share_used(got[:, held], ref.cols[:, held], ref.bound[:, held]) < 1.0
            vega = [pg.column(A, A + i, q, s) for i in range(A) for q in range(4) for s in (False, True)]
            assert np.all(got[:, vega] == 0.0)
