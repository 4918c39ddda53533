"""Sliced batched pricing (smc_gbm_price_sliced / BlackScholes.price_sliced): a contract cut into W slices, one
workgroup each, the six partial sums added in slice order by price_finish_kernel.

What is held bit for bit: one slice against smc_gbm_price | SMC_PRICE_REPLAY (f32 portable, f32 hw, f64; both schemes
and normalisations); the block run to run, under a split of the batch, with the ordinal on the host or the device, and
whatever the workspace held; in portable f32 math the raw terminal sum against the oracle's sliced row sum (span =
slice_paths, wg = 512) and the intrinsic values.  Within stated rounding bounds: the payoff means and standard errors
against the CPU restatement (tests/helpers/price_sliced_restate.py).  Within the a-priori bound of the independent
float64 reference (tests/helpers/gbm_reference.py), no element excluded: every column in portable, hw and f64 math.

The contracts are the twelve case rows of the CPU sweep (tests/test_gbm_reference.case_rows); every output buffer is
NaN-poisoned.  tests/test_price_sliced_reference.py holds the restatement to the same reference on the CPU and shares
its cached references with this file."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.effects import PathScheme
from spectralmc_amd.gbm import BlackScholes
from spectralmc_amd.models.numerical import Precision
from tests.helpers import gbm_reference as gref
from tests.helpers import instantiations as inst
from tests.helpers import (
    assert_rows_equal,
    expect_success,
    make_black_scholes_config,
    make_simulation_params,
    poisoned,
)
from tests.test_gbm_reference import ORD0, SEED, case_rows
from tests.test_price_sliced_reference import reference, restated

pytestmark = pytest.mark.gpu

DEV = "cuda"
COLS = _lib.PRICE_COLS
LOG, SIMPLE = gref.LOG_EULER, gref.SIMPLE_EULER
F32, F64 = _lib.DTYPE_F32, _lib.DTYPE_F64
HW, REPLAY = _lib.MATH_HW, _lib.PRICE_REPLAY
needs_longdouble = pytest.mark.skipif(not gref.LONGDOUBLE_OK, reason="numpy.longdouble has no 64-bit significand here")

# (T, P, slice_paths)
SLICED = [(16, 6837, 2048),   # W = 4: last slice of 693 paths, a partly valid lane and lanes wholly past P
          (5, 10241, 4096),   # W = 3: two chunks per slice, last slice of one path
          (1, 4624, 2048),    # W = 3: the 16-path stream span across slice boundaries
          (2, 4624, 2048)]    # W = 3: the same at T = 2
ONE = [(16, 4096, 4096),      # one slice of two chunks
       (16, 693, 2048)]       # one slice, P below the slice length
SIMPLE_CASE = (5, 6837, 2048)
# (T, P, slice_paths, scheme)
SLICED_CASES = [(*s, LOG) for s in SLICED] + [(*SIMPLE_CASE, SIMPLE)]
MATHS = {"portable": (0, F32), "hw": (HW, F32), "f64": (0, F64)}


def _rows(scheme: int = LOG, normalize: bool = True) -> np.ndarray:
    return case_rows(scheme, normalize)[0]


def _workspace(B: int, P: int, span: int, fill: float = float("nan"), extra: int = 0) -> torch.Tensor:
    need = int(_lib.lib().smc_gbm_price_sliced_workspace_bytes(B, P, span))
    assert need == 8 * B * (6 * -(-P // span) + 1)
    return torch.full((need // 8 + extra,), fill, dtype=torch.float64, device=DEV)


def _sliced(c: np.ndarray, T: int, P: int, span: int, scheme: int, norm: int, dtype: int = F32, ordinal0: int = ORD0,
            ordinal_dev: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> np.ndarray:
    B = c.shape[0]
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((B, COLS), torch.float64, DEV)
    ws = _workspace(B, P, span) if ws is None else ws
    _lib.check(_lib.lib().smc_gbm_price_sliced(_lib.ptr(cd), B, T, P, span, SEED, _lib.ptr(ordinal_dev), ordinal0,
                                               scheme, norm, dtype, _lib.ptr(out), _lib.ptr(ws), ws.numel() * 8, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _unsliced(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = F32, ordinal0: int = ORD0) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_price(_lib.ptr(cd), c.shape[0], T, P, SEED, None, ordinal0, scheme, norm, dtype,
                                        _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. one slice is the existing call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("T,P,span", ONE + [(5, 10241, 12288), (2, 4624, 1 << 20)])
def test_one_slice_is_the_unsliced_call(T, P, span, math) -> None:
    flag, dtype = MATHS[math]
    name = _lib.lib().smc_gbm_price_sliced_kernel
    for scheme in (LOG, SIMPLE):
        for norm in (0, 1):
            assert name(T, P, span, scheme | flag, norm, dtype).decode() == \
                f"price_slice_kernel({'replay' if norm else 'raw'})"
            c = _rows(scheme, bool(norm))
            want = _unsliced(c, T, P, scheme | flag | REPLAY, norm, dtype)
            got = _sliced(c, T, P, span, scheme | flag, norm, dtype)
            assert not np.isnan(want).any()
            assert_rows_equal(got, want, f"{math} T {T} P {P} slice {span} scheme {scheme} norm {norm}")


# ---- 2. fixed order ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("flag", [0, HW])
def test_sliced_is_deterministic_and_splits(flag, norm) -> None:
    T, P, span = SLICED[0]
    c = _rows(LOG, bool(norm))
    whole = _sliced(c, T, P, span, flag, norm, ordinal0=100)
    assert not np.isnan(whole).any()
    assert_rows_equal(_sliced(c, T, P, span, flag, norm, ordinal0=100), whole, "run to run")
    split = np.concatenate([_sliced(c[:5], T, P, span, flag, norm, ordinal0=100),
                            _sliced(c[5:], T, P, span, flag, norm, ordinal0=105)])
    assert_rows_equal(split, whole, "batch split at contract 5")
    # the ordinal's offset on the device, all of it and part of it
    for dev_part in (100, 40):
        od = torch.tensor([dev_part], dtype=torch.int64, device=DEV)
        assert_rows_equal(_sliced(c, T, P, span, flag, norm, ordinal0=100 - dev_part, ordinal_dev=od), whole,
                          f"ordinal_dev = {dev_part}")
    # an ordinal beyond 2^32, on the host against on the device
    far = (1 << 32) + 77
    host = _sliced(c, T, P, span, flag, norm, ordinal0=far)
    od = torch.tensor([1 << 32], dtype=torch.int64, device=DEV)
    assert_rows_equal(_sliced(c, T, P, span, flag, norm, ordinal0=77, ordinal_dev=od), host, "ordinal beyond 2^32")
    assert not np.array_equal(host[:, 7], _sliced(c, T, P, span, flag, norm, ordinal0=77)[:, 7])
    assert not np.array_equal(host[:, 7], whole[:, 7])
    # whatever the workspace held, and however much larger it is than needed
    B = c.shape[0]
    for label, ws in (("workspace of NaN", _workspace(B, P, span, float("nan"))),
                      ("workspace of zeros", _workspace(B, P, span, 0.0)),
                      ("larger workspace", _workspace(B, P, span, float("nan"), extra=4099))):
        assert_rows_equal(_sliced(c, T, P, span, flag, norm, ordinal0=100, ws=ws), whole, label)


# ---- 3. the terminal sum and the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("T,P,span,scheme", SLICED_CASES)
def test_sliced_matches_restatement_f32(T, P, span, scheme) -> None:
    e = P * 2.0 ** -52
    for norm in (0, 1):
        want = restated(T, P, span, scheme, bool(norm))
        w = want["cols"]
        got = _sliced(_rows(scheme, bool(norm)), T, P, span, scheme, norm)
        assert not np.isnan(got).any()
        # the oracle's sliced row sum (each slice in the 512-lane order, slices added in order) and the intrinsic
        # values: bit for bit
        assert_rows_equal(got[:, 7], w[:, 7], "terminal sum")
        assert_rows_equal(got[:, 5:7], w[:, 5:7], "intrinsic values")
        # two f64 sums of P non-negative terms in different orders each err by at most (P - 1) 2^-53 relative
        for col in range(3):
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(got[:, col] == w[:, col], 0.0, np.abs(got[:, col] - w[:, col]) / np.abs(w[:, col]))
            print(f"T {T} P {P} norm {norm} col {col}: max rel {rel.max():.3e} (bound {e:.3e})")
            np.testing.assert_allclose(got[:, col], w[:, col], rtol=e, atol=0, err_msg=f"col {col}")
        # tests/test_gpu_price.py's standard-error bound: D = sum v^2 - P m^2 moves by e (1 + 3 rho) D with rho =
        # m^2 / var, halved by the square root: 8 e max(1, rho / 2) relative.  A contract whose restated variance is
        # exactly zero (every payoff equal: v = 0, or out of the money on every path) has no relative bound: there
        # sum v^2 = P m^2 and each of the two moves by at most e of itself, so D <= 3 e P m^2 and the standard error
        # is at most |m| sqrt(3 e / (P - 1)) (0 where the mean is 0).
        rho = want["m2_over_var"]
        for col in (3, 4):
            tol = 8 * e * np.maximum(1.0, rho[:, col - 3] / 2)
            with np.errstate(invalid="ignore"):
                limit = np.where(w[:, col] > 0, tol * w[:, col], np.abs(w[:, col - 3]) * np.sqrt(3 * e / (P - 1)))
            err = np.abs(got[:, col] - w[:, col])
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.where(err == 0.0, 0.0, err / limit)
            print(f"T {T} P {P} norm {norm} col {col}: max share of its bound {share.max():.3f}")
            assert np.all(err <= limit), (col, int(np.argmax(share)))


# ---- 4. the independent reference --------------------------------------------------------------------------------------
def _check_reference(got: np.ndarray, ref: gref.GbmRef, label: str) -> None:
    assert not np.isnan(got).any(), label
    used = {"means": gref.share_used(got[:, :3], ref.price[:, :3], ref.price_bound[:, :3]),
            "stderr": gref.share_used(got[:, 3:5], ref.price[:, 3:5], ref.price_bound[:, 3:5]),
            "intrinsic": gref.share_used(got[:, 5:7], ref.price[:, 5:7], ref.price_bound[:, 5:7]),
            "terminal sum": gref.share_used(got[:, 7], ref.price[:, 7], ref.price_bound[:, 7])}
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) < 1.0, (label, used)


@pytest.mark.parametrize("math", ["portable", "hw"])
@pytest.mark.parametrize("T,P,span,scheme", SLICED_CASES)
def test_sliced_within_the_reference_bound_f32(T, P, span, scheme, math) -> None:
    flag, dtype = MATHS[math]
    # the calls the ledger counts for the row in this math: RAW (Raw, finish) and NORMALIZE (Sum, finish, Pay, finish)
    runs = [r for r in inst.pricing_runs_of("sliced f32", (T, P, span, scheme)) if r.math == math]
    assert [r.normalize for r in runs] == [False, True]
    for run in runs:
        normalize = run.normalize
        assert _lib.lib().smc_gbm_price_sliced_kernel(T, P, span, scheme | flag, int(normalize), dtype).decode() == run.name
        ref = reference(T, P, scheme, normalize, math)  # before the kernel's output is looked at
        got = _sliced(_rows(scheme, normalize), T, P, span, scheme | flag, int(normalize), dtype)
        _check_reference(got, ref, f"price_slice_kernel {math} T {T} P {P} slice {span} "
                                   f"{'log' if scheme == LOG else 'simple'} {'NORM' if normalize else 'RAW'}")


# (T, P, slice_paths, scheme): W = 3, last slice of 693 paths; the simple scheme's f64 instantiations at two slices
F64_SLICED_CASES = [(16, 4789, 2048, LOG), (5, 2741, 2048, SIMPLE)]


def _sliced_within_the_reference_bound_f64(T: int, P: int, span: int, scheme: int) -> None:
    _oracle.build()
    runs = inst.pricing_runs_of("sliced f64", (T, P, span, scheme))  # the calls the ledger counts for the row
    assert [r.normalize for r in runs] == [False, True]
    for run in runs:
        normalize = run.normalize
        assert _lib.lib().smc_gbm_price_sliced_kernel(T, P, span, scheme, int(normalize), F64).decode() == run.name
        rows = _rows(scheme, normalize)
        ref = gref.reference(_oracle, rows, T, P, SEED, ORD0, scheme=scheme, eps=gref.F64_ENGINE, normalize=normalize)
        got = _sliced(rows, T, P, span, scheme, int(normalize), F64)
        _check_reference(got, ref, f"price_slice_kernel f64 T {T} P {P} slice {span} "
                                   f"{'log' if scheme == LOG else 'simple'} {'NORM' if normalize else 'RAW'}")


@needs_longdouble
def test_sliced_within_the_reference_bound_f64() -> None:
    _sliced_within_the_reference_bound_f64(*F64_SLICED_CASES[0])


@needs_longdouble
def test_sliced_within_the_reference_bound_f64_simple_euler() -> None:
    _sliced_within_the_reference_bound_f64(*F64_SLICED_CASES[1])


# ---- 5. degenerate contracts and P = 1 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_sliced_degenerate_contracts(dtype) -> None:
    """v = 0 and T = 0 (tests/test_gpu_price.py's rows and bounds): every path ends on the forward, so the prices are
    the intrinsic values; with one slice the block is smc_gbm_price's bit for bit."""
    c = np.array([[100.0, 95.0, 2.0, 0.05, 0.01, 0.0], [50.0, 40.0, 0.0, 0.1, 0.0, 0.7],
                  [100.0, 120.0, 2.0, 0.05, 0.01, 0.0]])
    for T, P in ((8, 256), (3, 2053)):  # one slice; two, the second of 5 paths
        got = _sliced(c, T, P, 2048, LOG, 1, dtype, ordinal0=0)
        assert not np.isnan(got).any()
        F = c[:, 0] * np.exp((c[:, 3] - c[:, 4]) * c[:, 2])
        scale = np.maximum(c[:, 1], F)
        assert np.all(np.abs(got[:, 0] - got[:, 5]) <= 2.0 ** -22 * scale)
        assert np.all(np.abs(got[:, 1] - got[:, 6]) <= 2.0 ** -22 * scale)
        assert np.all(got[:, 3:5] <= 1e-6 * c[:, 1:2])
        assert got[1, 5] == 0.0 and got[1, 6] == 10.0 and got[1, 7] == 50.0 * P  # T = 0: exact
        assert got[0, 5] == 0.0 and got[2, 6] == 0.0 and got[0, 6] > 0 and got[2, 5] > 0
        if P <= 2048:
            assert_rows_equal(got, _unsliced(c, T, P, LOG | REPLAY, 1, dtype, ordinal0=0), "one slice")
        assert_rows_equal(_sliced(c, T, P, 4096, LOG, 1, dtype, ordinal0=0),
                          _unsliced(c, T, P, LOG | REPLAY, 1, dtype, ordinal0=0), "slice 4096: one slice")


@pytest.mark.parametrize("dtype", [F32, F64])
def test_sliced_single_path_has_zero_stderr(dtype) -> None:
    c = _rows(LOG, True)
    for norm in (0, 1):
        got = _sliced(c, 4, 1, 2048, LOG, norm, dtype)
        assert not np.isnan(got).any()
        assert np.all(got[:, 3:5] == 0.0)
        assert_rows_equal(got, _unsliced(c, 4, 1, LOG | REPLAY, norm, dtype), "P = 1")


# ---- 6. capturable -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0, 1])
def test_sliced_call_is_capturable(norm) -> None:
    T, P, span = SLICED[0]
    c = _rows(LOG, bool(norm))
    B = c.shape[0]
    eager = _sliced(c, T, P, span, LOG, norm)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((B, COLS), torch.float64, DEV)
    ws = _workspace(B, P, span)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        _lib.check(_lib.lib().smc_gbm_price_sliced(_lib.ptr(cd), B, T, P, span, SEED, None, ORD0, LOG, norm, F32,
                                                   _lib.ptr(out), _lib.ptr(ws), ws.numel() * 8, _lib.stream_handle()))
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())  # capturing launches nothing
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(out.cpu().numpy(), eager, "replayed graph vs eager")


# ---- 7. the Python API -------------------------------------------------------------------------------------------------
def _engine(dtype: Precision, T: int, N: int, M: int, scheme: PathScheme = PathScheme.LOG_EULER) -> BlackScholes:
    sp = make_simulation_params(timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, buffer_size=1,
                                skip=ORD0, dtype=dtype)
    return BlackScholes(make_black_scholes_config(sim_params=sp, path_scheme=scheme))


def _inputs(c: np.ndarray) -> list[BlackScholes.Inputs]:
    return [BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5]) for r in c.tolist()]


def _block(p: BlackScholes.BatchPrices) -> np.ndarray:
    names = ("put_price", "call_price", "underlying", "put_stderr", "call_stderr", "put_price_intrinsic",
             "call_price_intrinsic", "terminal_sum")
    for name in names:
        t = getattr(p, name)
        assert t.dtype == torch.float64 and t.is_cuda and t.ndim == 1, name
    return torch.stack([getattr(p, name) for name in names], dim=1).cpu().numpy()


@pytest.mark.parametrize("math", ["portable", "hw"])
def test_price_sliced_python_api(math) -> None:
    T, N, M = 16, 64, 64
    P = N * M  # 4096: the default slice is 2048, two slices
    c = _rows(LOG, True)
    B = c.shape[0]
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    flag = MATHS[math][0]
    L = _lib.lib()
    assert int(L.smc_gbm_price_slice_paths(P)) == 2048

    def engine() -> BlackScholes:
        e = _engine(Precision.float32, T, N, M)
        e.price_batch_math = math
        return e

    # the device form: the C call's bits, `served` advanced by B, the default slice through the query
    eng = engine()
    dev = _block(expect_success(eng.price_sliced_device(cd)))
    assert eng.ordinal == ORD0 + B
    assert_rows_equal(dev, _sliced(c, T, P, 2048, flag, 1), "price_sliced_device, default slice")
    nxt = _block(expect_success(eng.price_sliced_device(cd, slice_paths=2048)))
    assert eng.ordinal == ORD0 + 2 * B
    assert_rows_equal(nxt, _sliced(c, T, P, 2048, flag, 1, ordinal0=ORD0 + B), "the next B ordinals")
    empty = expect_success(eng.price_sliced_device(cd[:0]))
    assert empty.put_price.shape == (0,) and eng.ordinal == ORD0 + 2 * B
    assert expect_success(eng.price_sliced([])) == [] and eng.ordinal == ORD0 + 2 * B
    # the host form: one copy of the same block
    eng = engine()
    host = expect_success(eng.price_sliced(_inputs(c)))
    assert eng.ordinal == ORD0 + B and len(host) == B
    assert all(isinstance(h, BlackScholes.HostPricingResults) for h in host)
    assert [h.put_price for h in host] == dev[:, 0].tolist() and [h.call_price for h in host] == dev[:, 1].tolist()
    assert [h.underlying for h in host] == dev[:, 2].tolist()
    assert [h.put_price_intrinsic for h in host] == dev[:, 5].tolist()
    for h in host:
        assert h.put_convexity == h.put_price - h.put_price_intrinsic
        assert h.call_convexity == h.call_price - h.call_price_intrinsic
    # against price_batch: two slices agree with it within the reference's bound (the f64 sums are associated
    # differently), one slice bit for bit
    ref = reference(T, P, LOG, True, math)
    batch = _block(expect_success(engine().price_batch_device(cd)))
    assert np.all(np.abs(dev - batch) <= ref.price_bound), np.abs(dev - batch).max(axis=0)
    assert gref.share_used(dev, ref.price, ref.price_bound) < 1.0
    one = _block(expect_success(engine().price_sliced_device(cd, slice_paths=4096)))
    assert_rows_equal(one, batch, "one slice vs price_batch_device")
    assert [h.put_price for h in expect_success(engine().price_sliced(_inputs(c), slice_paths=4096))] == \
        [h.put_price for h in expect_success(engine().price_batch(_inputs(c)))]


def test_price_sliced_python_api_errors() -> None:
    from spectralmc_amd.errors.gbm import NormalsUnavailable
    from spectralmc_amd.result import Failure

    c = _rows(LOG, True)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    eng = _engine(Precision.float32, 16, 64, 64)
    # price_batch_device's validation errors
    with pytest.raises(ValueError, match="float64"):
        eng.price_sliced_device(cd.float())
    with pytest.raises(ValueError, match="float64"):
        eng.price_sliced_device(cd[:, :5])
    with pytest.raises(ValueError, match="device tensor"):
        eng.price_sliced_device(cd.cpu())
    with pytest.raises(ValueError, match="slice_paths"):
        eng.price_sliced_device(cd, slice_paths=1000)
    eng.price_batch_math = "fast"
    with pytest.raises(ValueError, match="price_batch_math"):
        eng.price_sliced_device(cd)
    assert eng.ordinal == ORD0
    # hardware math is a float32 mode: the f64 engine reports the C ABI's status
    e64 = _engine(Precision.float64, 8, 64, 64)
    e64.price_batch_math = "hw"
    with pytest.raises(_lib.SmcError) as exc:
        e64.price_sliced_device(cd)
    assert exc.value.code == _lib.SMC_ERR_INVALID_ARGUMENT and e64.ordinal == ORD0
    # an invalid normal buffer is the same Failure price_batch gives
    sp = make_simulation_params(timesteps=2, network_size=4, batches_per_mc_run=2, buffer_size=1000)
    bs = BlackScholes(make_black_scholes_config(sim_params=sp))
    one = bs.price_batch(_inputs(c)[:2])
    for res in (bs.price_sliced(_inputs(c)[:2]), bs.price_sliced([]), bs.price_sliced_device(cd[:2])):
        assert isinstance(res, Failure) and isinstance(res.error, NormalsUnavailable)
        assert res.error == one.error
    assert bs.ordinal == 0
