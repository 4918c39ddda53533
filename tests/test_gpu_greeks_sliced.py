"""Sliced batched Greeks (smc_gbm_greeks_sliced / BlackScholes.greeks_sliced): a contract cut into W slices, one
workgroup each, the 22 partial sums added in slice order by greeks_finish_kernel.

What is held bit for bit: one slice against smc_gbm_greeks | SMC_PRICE_REPLAY (f32 portable, f32 hw, f64; both
normalisations); columns 20..24 against smc_gbm_price_sliced's 0, 1, 3, 4, 7 at the same slice length, at any W; the
block run to run, under a split of the batch, with the ordinal on the host or the device, and whatever the workspace
held; in portable f32 math the raw terminal sum against the oracle's sliced row sum.  Within stated rounding bounds:
the means and standard errors against the CPU restatement (tests/helpers/greeks_sliced_restate.py).  Within the a-priori
bound of the independent float64 reference (tests/helpers/greeks_reference.py): every column in portable and hw math;
f64 at the project's float64 tolerance.

The contracts are the fourteen case rows of the CPU sweep (tests/test_greeks_reference.case_rows) and its degenerate
rows; every output buffer is NaN-poisoned and the workspace NaN-filled.  tests/test_greeks_sliced_reference.py holds
the restatement to the same reference on the CPU and shares its cached references with this file."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.effects import ForwardNormalization, PathScheme
from spectralmc_amd.gbm import BlackScholes
from spectralmc_amd.models.numerical import Precision
from tests.helpers import (
    ATOL_FLOAT64,
    RTOL_FLOAT64,
    assert_rows_equal,
    expect_success,
    make_black_scholes_config,
    make_simulation_params,
    poisoned,
)
from tests.helpers import gbm_reference as gref
from tests.helpers import greeks_reference as gk
from tests.helpers import greeks_restate as restate
from tests.helpers import greeks_sliced_restate as gsr
from tests.test_greeks_reference import ORD0, SEED, case_rows, degenerate_rows
from tests.test_greeks_sliced_reference import SLICED, reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
COLS = _lib.GREEKS_COLS
F32, F64 = _lib.DTYPE_F32, _lib.DTYPE_F64
HW, REPLAY = _lib.MATH_HW, _lib.PRICE_REPLAY
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
MATHS = {"portable": (0, F32), "hw": (HW, F32), "f64": (0, F64)}
MEANS = list(range(10))
NAMES = ["put_delta", "call_delta", "put_vega", "call_vega", "put_rho", "call_rho", "put_theta", "call_theta",
         "put_gamma", "call_gamma"]
STDERR_COLS = list(range(10, 20)) + [22, 23]


def _workspace(B: int, P: int, span: int, fill: float = float("nan"), extra: int = 0) -> torch.Tensor:
    need = int(_lib.lib().smc_gbm_greeks_sliced_workspace_bytes(B, P, span))
    assert need == 8 * B * (22 * -(-P // span) + 2)
    return torch.full((need // 8 + extra,), fill, dtype=torch.float64, device=DEV)


def _sliced(c: np.ndarray, T: int, P: int, span: int, scheme: int, norm: int, dtype: int = F32, ordinal0: int = ORD0,
            ordinal_dev: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> np.ndarray:
    B = c.shape[0]
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((B, COLS), torch.float64, DEV)
    ws = _workspace(B, P, span) if ws is None else ws
    _lib.check(_lib.lib().smc_gbm_greeks_sliced(_lib.ptr(cd), B, T, P, span, SEED, _lib.ptr(ordinal_dev), ordinal0,
                                                scheme, norm, dtype, _lib.ptr(out), _lib.ptr(ws), ws.numel() * 8, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _unsliced(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = F32, ordinal0: int = ORD0) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_greeks(_lib.ptr(cd), c.shape[0], T, P, SEED, None, ordinal0, scheme, norm, dtype,
                                         _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _price_sliced(c: np.ndarray, T: int, P: int, span: int, scheme: int, norm: int, dtype: int) -> np.ndarray:
    B = c.shape[0]
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((B, _lib.PRICE_COLS), torch.float64, DEV)
    need = int(_lib.lib().smc_gbm_price_sliced_workspace_bytes(B, P, span))
    ws = torch.full((need // 8,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().smc_gbm_price_sliced(_lib.ptr(cd), B, T, P, span, SEED, None, ORD0, scheme, norm, dtype,
                                               _lib.ptr(out), _lib.ptr(ws), need, None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_name(T: int, P: int, span: int, scheme: int, norm: int, dtype: int) -> None:
    got = _lib.lib().smc_gbm_greeks_sliced_kernel(T, P, span, scheme, norm, dtype).decode()
    assert got == f"greeks_slice_kernel({'replay' if norm else 'raw'})", got


# ---- 1. one slice is the unsliced call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("T,P,span", [(16, 4096, 4096), (16, 693, 2048), (5, 10241, 12288), (2, 4624, 1 << 20)])
def test_one_slice_is_the_unsliced_call(T, P, span, math) -> None:
    flag, dtype = MATHS[math]
    c = case_rows()
    for norm in (RAW, NORM):
        _assert_name(T, P, span, flag, norm, dtype)
        assert _lib.lib().smc_gbm_greeks_kernel(T, P, flag | REPLAY, norm, dtype).decode() == \
            f"greeks_kernel({'replay' if norm else 'raw'})"
        want = _unsliced(c, T, P, flag | REPLAY, norm, dtype)
        got = _sliced(c, T, P, span, flag, norm, dtype)
        assert not np.isnan(want).any()
        assert_rows_equal(got, want, f"{math} T {T} P {P} slice {span} norm {norm}")


# ---- 2. the price columns are the sliced price call's ------------------------------------------------------------------
@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("T,P,span", SLICED)
def test_price_columns_are_the_sliced_price_call(T, P, span, math) -> None:
    flag, dtype = MATHS[math]
    c = case_rows()
    for norm in (RAW, NORM):
        _assert_name(T, P, span, flag, norm, dtype)
        got = _sliced(c, T, P, span, flag, norm, dtype)
        price = _price_sliced(c, T, P, span, flag, norm, dtype)
        assert not np.isnan(got).any() and not np.isnan(price).any()
        assert_rows_equal(got[:, 20:25], price[:, [0, 1, 3, 4, 7]],
                          f"{math} T {T} P {P} slice {span} norm {norm}: columns 20..24 vs the sliced price call")
        if norm == RAW:
            assert np.all(got[:, 25] == 0.0)


# ---- 3. fixed order ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [RAW, NORM])
@pytest.mark.parametrize("flag", [0, HW])
def test_sliced_is_deterministic_and_splits(flag, norm) -> None:
    T, P, span = SLICED[0]
    c = case_rows()
    _assert_name(T, P, span, flag, norm, F32)
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
    assert not np.array_equal(host[:, 24], _sliced(c, T, P, span, flag, norm, ordinal0=77)[:, 24])
    assert not np.array_equal(host[:, 24], whole[:, 24])
    # whatever the workspace held, and however much larger it is than needed
    B = c.shape[0]
    for label, ws in (("workspace of NaN", _workspace(B, P, span, float("nan"))),
                      ("workspace of zeros", _workspace(B, P, span, 0.0)),
                      ("larger workspace", _workspace(B, P, span, float("nan"), extra=4099))):
        assert_rows_equal(_sliced(c, T, P, span, flag, norm, ordinal0=100, ws=ws), whole, label)


# ---- 4. the independent reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["portable", "hw"])
@pytest.mark.parametrize("T,P,span", SLICED)
def test_sliced_within_the_reference_bound_f32(T, P, span, math) -> None:
    flag, dtype = MATHS[math]
    c = case_rows()
    for norm in (RAW, NORM):
        _assert_name(T, P, span, flag, norm, dtype)
        ref = reference(T, P, norm == NORM, math)  # before the kernel's output is looked at
        assert gref.count_ok(ref.doubt, P), ref.doubt  # the condition on the strikes, on the reference alone
        got = _sliced(c, T, P, span, flag, norm, dtype)
        label = f"greeks_slice_kernel {math} T {T} P {P} slice {span} {'NORM' if norm else 'RAW'}"
        assert got.shape == (c.shape[0], gk.COLS) and not np.isnan(got).any(), label
        used = gk.shares(got, ref)
        print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
              + f"; paths in doubt {int(ref.doubt.max())}")
        assert max(used.values()) < 1.0, (label, used)


# ---- 5. portable f32 against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,P,span", SLICED)
def test_sliced_matches_restatement_f32(T, P, span) -> None:
    """tests/test_gpu_greeks.py's tolerances for greeks_kernel: the raw terminal sum bit for bit (here the oracle's
    sliced row sum), every other sum within the P 2^-52 bound of two f64 sums of the same terms in different orders."""
    _oracle.build()
    c = case_rows()
    term, L, tsum = gsr.paths_f32(_oracle, c, T, P, span, SEED, ORD0)
    xl = (term * L).astype(np.float64)
    vt = c[:, 5] * c[:, 2]
    with np.errstate(divide="ignore"):
        inv_den = np.where(vt == 0, 0.0, 1.0 / (vt * c[:, 0] * c[:, 0]))  # gamma is 0 where v T == 0
    for norm in (RAW, NORM):
        _assert_name(T, P, span, 0, norm, F32)
        got = _sliced(c, T, P, span, 0, norm)
        assert not np.isnan(got).any()
        assert_rows_equal(got[:, 24], tsum, "terminal sum")
        if norm:
            want_xl, bound_xl = xl.sum(axis=1), P * 2.0 ** -52 * np.abs(xl).sum(axis=1)
            err_xl = np.abs(got[:, 25] - want_xl)
            with np.errstate(divide="ignore", invalid="ignore"):
                print(f"sumxl: max share of its bound {np.max(np.where(err_xl == 0, 0.0, err_xl / bound_xl)):.3e}")
            assert np.all(err_xl <= bound_xl)
        else:
            assert np.all(got[:, 25] == 0.0)
        # Lbar from the kernel's own columns 24 and 25, as tests/test_gpu_greeks.py takes it
        with np.errstate(divide="ignore", invalid="ignore"):
            r = restate.terms(c, term, norm, got[:, 24], got[:, 25], L)
            s = restate.summary(r["t"], c)
        w = s["cols"]
        for col in MEANS:
            err, bound = np.abs(got[:, col] - w[:, col]), s["bound"][col]
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.where(err == 0, 0.0, err / bound)
            print(f"{NAMES[col]}: max share of its bound {share.max():.3e}")
            assert np.all(err <= bound), (NAMES[col], int(np.argmax(share)))
        for i, col in enumerate((20, 21)):
            assert np.all(np.abs(got[:, col] - w[:, col]) <= s["price_bound"][i]), col
        for term_i in range(8):
            restate.check_stderr(got[:, 10 + term_i], w[:, 10 + term_i], s, term_i, P, NAMES[term_i])
        for i in range(2):  # gamma's error is vega's over v T X0^2, the prices' are columns 22, 23
            restate.check_stderr(got[:, 18 + i], w[:, 18 + i], s, 2 + i, P, NAMES[8 + i], scale=inv_den)
            restate.check_stderr(got[:, 22 + i], w[:, 22 + i], s, 8 + i, P, ("put", "call")[i])


# ---- 6. f64 ------------------------------------------------------------------------------------------------------------
def test_sliced_f64_against_the_reference() -> None:
    """The existing f64 Greeks test's criterion (tests/test_gpu_greeks_reference.py) at W = 3, last slice of 693 paths."""
    _oracle.build()
    T, P, span = 16, 4789, 2048
    c = case_rows()
    for norm in (RAW, NORM):
        _assert_name(T, P, span, 0, norm, F64)
        ref = gk.reference(_oracle, c, T, P, SEED, ORD0, normalize=norm == NORM, f64=True)
        got = _sliced(c, T, P, span, 0, norm, F64)
        assert not np.isnan(got).any()
        share = np.abs(got - ref.cols) / gk.tol64(ref, RTOL_FLOAT64, ATOL_FLOAT64)
        print(f"greeks_slice_kernel f64 T {T} P {P} slice {span} {'NORM' if norm else 'RAW'}: largest share of the f64 "
              f"tolerance {share.max():.3e} (column {int(share.max(axis=0).argmax())})")
        assert np.all(share <= 1.0), np.argwhere(share > 1.0).tolist()


# ---- 7. degenerate rows and P = 1 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [RAW, NORM])
def test_sliced_degenerate_rows_within_the_bound(norm) -> None:
    """v = 0 (vega, gamma and their errors exactly 0), the T v^2 corner, the flat row, T = 0 and v = 0.01, as
    test_greeks_kernel_degenerate_rows_within_the_bound lists them, at W = 3 (last slice of 256 paths)."""
    _oracle.build()
    rows = degenerate_rows()
    T, P, span = 8, 4352, 2048
    for math in ("portable", "hw"):
        flag, dtype = MATHS[math]
        _assert_name(T, P, span, flag, norm, dtype)
        ref = gk.reference(_oracle, rows, T, P, SEED, ORD0, math=math, normalize=norm == NORM)
        assert gref.count_ok(ref.doubt, P) and int(ref.doubt.max()) == 0, ref.doubt
        got = _sliced(rows, T, P, span, flag, norm, dtype)
        assert not np.isnan(got).any()
        used = gk.shares(got, ref)
        print(f"greeks_slice_kernel degenerate rows {math} {'NORM' if norm else 'RAW'}: share of the bound used "
              + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
        assert max(used.values()) < 1.0, (math, used)
        assert np.all(got[[0, 2]][:, [2, 3, 8, 9, 12, 13, 18, 19]] == 0.0)  # v == 0
        assert np.all(got[3, [8, 9, 18, 19]] == 0.0)                        # T == 0
        if norm == RAW:
            assert np.all(got[:, 25] == 0.0)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_sliced_single_path_has_zero_stderr(dtype) -> None:
    c = case_rows()
    for norm in (RAW, NORM):
        _assert_name(4, 1, 2048, 0, norm, dtype)
        got = _sliced(c, 4, 1, 2048, 0, norm, dtype)
        assert not np.isnan(got).any()
        assert np.all(got[:, STDERR_COLS] == 0.0)
        assert_rows_equal(got, _unsliced(c, 4, 1, REPLAY, norm, dtype), "P = 1")


# ---- 8. capturable -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [RAW, NORM])
def test_sliced_call_is_capturable(norm) -> None:
    """A linear chain of two (RAW) or four (NORMALIZE) kernels on one stream: no parallel branches."""
    T, P, span = SLICED[0]
    c = case_rows()
    B = c.shape[0]
    _assert_name(T, P, span, 0, norm, F32)
    eager = _sliced(c, T, P, span, 0, norm)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((B, COLS), torch.float64, DEV)
    ws = _workspace(B, P, span)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        _lib.check(_lib.lib().smc_gbm_greeks_sliced(_lib.ptr(cd), B, T, P, span, SEED, None, ORD0, 0, norm, F32,
                                                    _lib.ptr(out), _lib.ptr(ws), ws.numel() * 8, _lib.stream_handle()))
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all())  # capturing launches nothing
    for replay in range(2):
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_rows_equal(out.cpu().numpy(), eager, f"replay {replay} of the graph vs eager")


# ---- 9. the Python API -------------------------------------------------------------------------------------------------
def _engine(dtype: Precision, T: int, N: int, M: int, scheme: PathScheme = PathScheme.LOG_EULER,
            norm: ForwardNormalization = ForwardNormalization.NORMALIZE) -> BlackScholes:
    sp = make_simulation_params(timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, buffer_size=1,
                                skip=ORD0, dtype=dtype)
    return BlackScholes(make_black_scholes_config(sim_params=sp, path_scheme=scheme, normalization=norm))


def _inputs(c: np.ndarray) -> list[BlackScholes.Inputs]:
    return [BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5]) for r in c.tolist()]


FIELDS = list(BlackScholes.BatchGreeks.model_fields)


def _block(g: BlackScholes.BatchGreeks) -> np.ndarray:
    for name in FIELDS:
        t = getattr(g, name)
        assert t.dtype == torch.float64 and t.is_cuda and t.ndim == 1, name
    return torch.stack([getattr(g, name) for name in FIELDS], dim=1).cpu().numpy()


@pytest.mark.parametrize("math", ["portable", "hw"])
def test_greeks_sliced_python_api(math) -> None:
    T, N, M = 16, 64, 64
    P = N * M  # 4096: the default slice is 2048, two slices
    c = case_rows()
    B = c.shape[0]
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    flag = MATHS[math][0]
    assert len(FIELDS) == COLS
    assert int(_lib.lib().smc_gbm_price_slice_paths(P)) == 2048
    _assert_name(T, P, 2048, flag, NORM, F32)

    def engine() -> BlackScholes:
        e = _engine(Precision.float32, T, N, M)
        e.price_batch_math = math
        return e

    # the device form: the C call's bits on the same ordinals, `served` advanced by B, the default slice from the query
    eng = engine()
    dev = _block(expect_success(eng.greeks_sliced_device(cd)))
    assert eng.ordinal == ORD0 + B
    assert_rows_equal(dev, _sliced(c, T, P, 2048, flag, NORM), "greeks_sliced_device, default slice")
    nxt = _block(expect_success(eng.greeks_sliced_device(cd, slice_paths=2048)))
    assert eng.ordinal == ORD0 + 2 * B
    assert_rows_equal(nxt, _sliced(c, T, P, 2048, flag, NORM, ordinal0=ORD0 + B), "the next B ordinals")
    empty = expect_success(eng.greeks_sliced_device(cd[:0]))
    assert all(getattr(empty, name).shape == (0,) for name in FIELDS) and eng.ordinal == ORD0 + 2 * B
    assert expect_success(eng.greeks_sliced([])) == [] and eng.ordinal == ORD0 + 2 * B
    # the host form: one copy of the same block
    eng = engine()
    host = expect_success(eng.greeks_sliced(_inputs(c)))
    assert eng.ordinal == ORD0 + B and len(host) == B
    assert all(isinstance(h, BlackScholes.HostGreeks) for h in host)
    for i, name in enumerate(FIELDS):
        assert_rows_equal(np.array([getattr(h, name) for h in host]), dev[:, i], name)
    # against greeks_batch_device: one slice bit for bit
    batch = _block(expect_success(engine().greeks_batch_device(cd)))
    one = _block(expect_success(engine().greeks_sliced_device(cd, slice_paths=4096)))
    assert_rows_equal(one, batch, "one slice vs greeks_batch_device")
    host_one = expect_success(engine().greeks_sliced(_inputs(c), slice_paths=4096))
    host_batch = expect_success(engine().greeks_batch(_inputs(c)))
    assert [h.put_delta for h in host_one] == [h.put_delta for h in host_batch]
    assert [h.call_vega for h in host_one] == [h.call_vega for h in host_batch]


def test_greeks_sliced_python_api_errors() -> None:
    from spectralmc_amd.errors.gbm import NormalsUnavailable
    from spectralmc_amd.result import Failure

    c = case_rows()
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    eng = _engine(Precision.float32, 16, 64, 64)
    with pytest.raises(ValueError, match="float64"):
        eng.greeks_sliced_device(cd.float())
    with pytest.raises(ValueError, match="float64"):
        eng.greeks_sliced_device(cd[:, :5])
    with pytest.raises(ValueError, match="device tensor"):
        eng.greeks_sliced_device(cd.cpu())
    for bad in (1000, 0, -2048):
        with pytest.raises(ValueError, match="slice_paths"):
            eng.greeks_sliced_device(cd, slice_paths=bad)
    with pytest.raises(ValueError, match="slice_paths"):
        eng.greeks_sliced(_inputs(c), slice_paths=1000)
    eng.price_batch_math = "fast"
    with pytest.raises(ValueError, match="price_batch_math"):
        eng.greeks_sliced_device(cd)
    assert eng.ordinal == ORD0
    # a simple-Euler engine raises, in both forms
    simple = _engine(Precision.float32, 16, 64, 64, scheme=PathScheme.SIMPLE_EULER)
    with pytest.raises(ValueError, match="SIMPLE_EULER"):
        simple.greeks_sliced_device(cd)
    with pytest.raises(ValueError, match="SIMPLE_EULER"):
        simple.greeks_sliced(_inputs(c))
    assert simple.ordinal == ORD0
    # hardware math is a float32 mode: the f64 engine reports the C ABI's status and consumes nothing
    e64 = _engine(Precision.float64, 8, 64, 64)
    e64.price_batch_math = "hw"
    with pytest.raises(_lib.SmcError) as exc:
        e64.greeks_sliced_device(cd)
    assert exc.value.code == _lib.SMC_ERR_INVALID_ARGUMENT and e64.ordinal == ORD0
    # an invalid normal buffer is the same Failure greeks_batch gives
    sp = make_simulation_params(timesteps=2, network_size=4, batches_per_mc_run=2, buffer_size=1000)
    bs = BlackScholes(make_black_scholes_config(sim_params=sp))
    one = bs.greeks_batch(_inputs(c)[:2])
    for res in (bs.greeks_sliced(_inputs(c)[:2]), bs.greeks_sliced([]), bs.greeks_sliced_device(cd[:2])):
        assert isinstance(res, Failure) and isinstance(res.error, NormalsUnavailable)
        assert res.error == one.error
    assert bs.ordinal == 0
