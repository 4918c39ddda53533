"""path_greeks_kernel (smc_gbm_greeks_paths) within the a-priori bound of the independent reference
(tests/helpers/path_greeks_reference.py): the f32 kernel in portable and in SMC_MATH_HW math, RAW and NORMALIZE, and
the f64 kernel against the reference evaluated in long double.  At one time step the Asian and lookback columns are
smc_gbm_greeks' European ones within the sum of the two references' bounds.  The inputs (tests/helpers/
path_greeks_cases.py) keep the bounds from being vacuous: tests/test_path_greeks_reference.py asserts the caps on the
paths in doubt, and they are asserted again here for the typing of each case."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from tests.helpers import gbm_reference as gref
from tests.helpers import greeks_reference as gk
from tests.helpers import instantiations as inst
from tests.helpers import path_greeks_reference as pg
from tests.helpers import poisoned
from tests.helpers.path_greeks_cases import CASES, FLAT_ROWS, ORD0, ROWS, SEED

pytestmark = pytest.mark.gpu

DEV = "cuda"
# math -> (scheme flags, dtype)
MODES = {"portable": (0, 0), "hw": (_lib.MATH_HW, 0), "f64": (0, 1)}


def _call(fn, cols: int, c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], cols), torch.float64, DEV)
    _lib.check(fn(_lib.ptr(cd), c.shape[0], T, P, SEED, None, ORD0, scheme, norm, dtype, _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _greeks(c: np.ndarray, T: int, P: int, math: str, norm: int) -> np.ndarray:
    scheme, dtype = MODES[math]
    return _call(_lib.lib().smc_gbm_greeks_paths, _lib.PATH_GREEKS_COLS, c, T, P, scheme, norm, dtype)


@functools.lru_cache(maxsize=None)
def _ref(T: int, P: int, norm: int, math: str) -> pg.PathGreeksRef:
    _oracle.build()
    return pg.reference(_oracle, ROWS, T, P, SEED, ORD0, math=math, normalize=bool(norm))


# the shapes of the CPU test, and per dtype the T whose NORMALIZE plan is three sweeps with a short last one
SHAPES = {"portable": CASES + [(37, 693)], "hw": CASES + [(37, 693)], "f64": CASES + [(29, 693)]}


# (math, T, P): tests/test_instantiation_ledger.py holds the table to the ledger of instantiations
SHAPE_CASES = [(m, T, P) for m in MODES for T, P in SHAPES[m]]


@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("math,T,P", SHAPE_CASES)
def test_path_greeks_within_the_reference_bound(math, T, P, norm) -> None:
    if math == "f64" and not gref.LONGDOUBLE_OK:
        pytest.skip("the f64 kernel's reference needs a long double with a 64-bit significand")
    # the launch is one the ledger counts for the row, under the name the library's query gives it
    run, = (r for r in inst.pricing_runs_of("path greeks", (math, T, P)) if r.normalize == bool(norm))
    assert (run.dtype, run.math) == (("f64", "portable") if math == "f64" else ("f32", math))
    assert _lib.lib().smc_gbm_greeks_paths_kernel(T, P, MODES[math][0], norm, MODES[math][1]).decode() == run.name
    ref = _ref(T, P, norm, math)
    assert gref.count_ok(ref.doubt_ind, P) and pg.arg_ok(ref.doubt_arg, P)
    got = _greeks(ROWS, T, P, math, norm)
    assert np.isfinite(got).all()
    for name, cols in (("means", pg.MEAN_COLS), ("stderr", pg.STDERR_COLS)):
        want, bound = ref.cols[:, cols].astype(np.float64), ref.bound[:, cols].astype(np.float64)
        share = gref.share_used(got[:, cols], want, bound)
        print(f"{math} T {T} P {P} norm {norm} {name}: largest share of the bound {share:.3f}")
        assert share <= 1.0, name


@pytest.mark.parametrize("math", ["portable", "hw"])
@pytest.mark.parametrize("norm", [0, 1])
def test_flat_row_delta_and_rho_within_the_bound(math, norm) -> None:
    """v = 0 and r = d: every row is X0 and ties; the first row wins.  Held on delta and rho, as the vega and theta
    of such a row are conventions."""
    _oracle.build()
    T, P = 5, 693
    ref = pg.reference(_oracle, FLAT_ROWS, T, P, SEED, ORD0, math=math, normalize=bool(norm))
    assert not ref.doubt_arg.any() and not ref.doubt_ind.any()
    got = _greeks(FLAT_ROWS, T, P, math, norm)
    cols = [pg.column(g, q) for g in (0, 2) for q in range(4)]
    assert np.all(np.abs(got[:, cols] - ref.cols[:, cols]) <= ref.bound[:, cols])


@pytest.mark.parametrize("math", ["portable", "hw"])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("P", [1, 693, 2048])
def test_one_time_step_is_the_european_greeks(math, norm, P) -> None:
    """T = 1: the average, the maximum and the minimum are the terminal value, so delta, vega, rho and theta of the
    Asian and of the lookback pair are smc_gbm_greeks' columns 0..7, each kernel within its own reference's bound of
    the one model value."""
    _oracle.build()
    scheme, dtype = MODES[math]
    got = _greeks(ROWS, 1, P, math, norm)
    eur = _call(_lib.lib().smc_gbm_greeks, _lib.GREEKS_COLS, ROWS, 1, P, scheme, norm, dtype)
    ref = pg.reference(_oracle, ROWS, 1, P, SEED, ORD0, math=math, normalize=bool(norm))
    eref = gk.reference(_oracle, ROWS, 1, P, SEED, ORD0, math=math, normalize=bool(norm))
    for g in range(4):
        for q in range(4):
            a, e = pg.column(g, q), 2 * g + (q & 1)
            model = np.abs(ref.cols[:, a] - eref.cols[:, e])           # the two references state one model
            assert np.all(model <= 1e-12 * (1.0 + np.abs(eref.cols[:, e]))), (g, q)
            assert np.all(np.abs(got[:, a] - eur[:, e]) <= ref.bound[:, a] + eref.bound[:, e] + model), (g, q)
            b, f = pg.column(g, q, True), 10 + 2 * g + (q & 1)
            model = np.abs(ref.cols[:, b] - eref.cols[:, f])
            assert np.all(model <= 1e-12 * (1.0 + np.abs(eref.cols[:, f]))), (g, q)
            assert np.all(np.abs(got[:, b] - eur[:, f]) <= ref.bound[:, b] + eref.bound[:, f] + model), (g, q)
