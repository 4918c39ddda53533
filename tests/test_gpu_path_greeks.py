"""Batched Greeks of the Asian and lookback options (smc_gbm_greeks_paths / BlackScholes.greeks_paths_batch): the
[B][40] block of path_greeks_kernel against the CPU restatement of the table in include/spectralmc_hip.h
(tests/helpers/path_greeks_restate.py).  The restatement takes its sums in the kernel's own order, so the portable
f32 block is held to it bit for bit, every column; the price columns are held to smc_gbm_price_paths bit for bit in
both dtypes; the block is bit-identical run to run, under a split of the batch, with the ordinal on the device and
across sweep counts.  The independent float64 reference is tests/test_gpu_path_greeks_reference.py's."""

from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from spectralmc_amd import _lib
from spectralmc_amd.effects import ForwardNormalization, PathScheme
from spectralmc_amd.gbm import BlackScholes
from spectralmc_amd.models.numerical import Precision
from tests.helpers import (
    assert_rows_equal,
    expect_success,
    make_black_scholes_config,
    make_simulation_params,
    poisoned,
)
from tests.helpers import path_greeks_restate as restate
from tests.helpers.gbm_restate import contracts as _contracts

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7
ORD0 = 11
COLS = _lib.PATH_GREEKS_COLS
PRICE_FROM = [0, 1, 4, 5, 8, 9, 12, 13]   # smc_gbm_price_paths' columns behind columns 32..39
STDERR_COLS = list(range(16, 32)) + [36, 37, 38, 39]
# a T per dtype whose NORMALIZE plan is three sweeps with a short last one (16 + 16 + 5 and 12 + 12 + 5)
T_THREE_SWEEPS = {0: 37, 1: 29}


def _greeks(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = 0, ordinal0: int = ORD0,
            seed: int = SEED, ordinal_dev: torch.Tensor | None = None) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_greeks_paths(_lib.ptr(cd), c.shape[0], T, P, seed, _lib.ptr(ordinal_dev), ordinal0,
                                               scheme, norm, dtype, _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _prices(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = 0, ordinal0: int = ORD0) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], _lib.PATH_PRICE_COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_price_paths(_lib.ptr(cd), None, c.shape[0], T, P, SEED, None, ordinal0, scheme, norm,
                                              dtype, _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _sweeps(T: int, norm: int, dtype: int) -> int:
    rows, lds = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.lib().smc_test_path_greeks_plan(T, 0, norm, dtype, ctypes.byref(rows), ctypes.byref(lds)))
    return -(-T // rows.value) if norm else 1


@functools.lru_cache(maxsize=None)
def _want_f32(B: int, T: int, P: int, norm: int) -> np.ndarray:
    out = restate.block_f32(_contracts(B), T, P, SEED, ORD0, norm)
    out.setflags(write=False)
    return out


# --------------------------------------------------------------------------- 1. restatement, portable f32, bit for bit
# (B, T, P): odd T and ragged P; two whole chunks and a full sweep; the three-sweep T; T = 1 and 2; one path
F32_CASES = [(12, 5, 693), (12, 16, 4096), (3, T_THREE_SWEEPS[0], 693), (12, 1, 2048), (12, 2, 693), (12, 5, 1)]


@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("B,T,P", F32_CASES)
def test_path_greeks_match_restatement_bitwise_f32(B, T, P, norm) -> None:
    c = _contracts(B)
    got = _greeks(c, T, P, 0, norm)
    assert not np.isnan(got).any()
    name = _lib.lib().smc_gbm_greeks_paths_kernel(T, P, 0, norm, 0).decode()
    assert name == ("path_greeks_kernel(replay)" if norm else "path_greeks_kernel(raw)")
    if T == T_THREE_SWEEPS[0]:
        assert _sweeps(T, 1, 0) == 3 and T % 16 not in (0, 15)
    want = _want_f32(B, T, P, norm)
    for col in range(COLS):
        assert_rows_equal(got[:, col], want[:, col], f"column {col}")
    if P == 1:
        assert np.all(got[:, STDERR_COLS] == 0.0)


# --------------------------------------------------------------------------- 2. the price columns are the price call's
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("T,P", [(5, 693), (16, 4096), (1, 2048)])
def test_path_greeks_price_columns_are_the_price_call(T, P, norm, dtype) -> None:
    c = _contracts(12)
    got = _greeks(c, T, P, 0, norm, dtype)
    price = _prices(c, T, P, 0, norm, dtype)
    for i, src in enumerate(PRICE_FROM):
        assert_rows_equal(got[:, 32 + i], price[:, src], f"column {32 + i} vs price column {src}")


def test_path_greeks_price_columns_hw_math() -> None:
    c = _contracts(12)
    got = _greeks(c, 16, 4096, _lib.MATH_HW, 1)
    price = _prices(c, 16, 4096, _lib.MATH_HW, 1)
    for i, src in enumerate(PRICE_FROM):
        assert_rows_equal(got[:, 32 + i], price[:, src], f"column {32 + i} vs price column {src}")


# --------------------------------------------------------------------------- 3. run to run, split, device ordinal
@pytest.mark.parametrize("dtype,scheme", [(0, 0), (0, _lib.MATH_HW), (1, 0)])
def test_path_greeks_are_deterministic_and_split(dtype, scheme) -> None:
    c = _contracts(12)
    T, P = 16, 4096
    whole = _greeks(c, T, P, scheme, 1, dtype, 100)
    assert not np.isnan(whole).any()
    assert_rows_equal(_greeks(c, T, P, scheme, 1, dtype, 100), whole, "run to run")
    assert_rows_equal(_greeks(c[5:], T, P, scheme, 1, dtype, 105), whole[5:], "batch split at contract 5")
    assert_rows_equal(_greeks(c[:5], T, P, scheme, 1, dtype, 100), whole[:5], "batch split at contract 5, the head")
    for dev_part in (105, 40):
        od = torch.tensor([dev_part], dtype=torch.int64, device=DEV)
        assert_rows_equal(_greeks(c[5:], T, P, scheme, 1, dtype, 105 - dev_part, ordinal_dev=od), whole[5:],
                          f"ordinal_dev = {dev_part}")
    assert not np.array_equal(_greeks(c, T, P, scheme, 1, dtype, 101)[:, 0], whole[:, 0])  # other ordinals


# --------------------------------------------------------------------------- 4. sweep counts
def test_path_greeks_sweep_boundaries_change_nothing_f64() -> None:
    """The sweep count cannot be forced from outside; in f32 the three-sweep T is held to the restatement above.  In
    f64 the plan gives T = 16 two sweeps (12 + 4) and T = 29 three (12 + 12 + 5): a row's two sums lie in one sweep,
    so the NORMALIZE price columns still equal smc_gbm_price_paths' (whose plan covers both T in other sweeps: its
    accumulator rows are half as wide), bit for bit, and the RAW and NORMALIZE blocks are finite."""
    assert _sweeps(16, 1, 1) == 2 and _sweeps(T_THREE_SWEEPS[1], 1, 1) == 3
    c = _contracts(3)
    T, P = T_THREE_SWEEPS[1], 693
    got = _greeks(c, T, P, 0, 1, 1)
    assert np.isfinite(got).all()
    price = _prices(c, T, P, 0, 1, 1)
    for i, src in enumerate(PRICE_FROM):
        assert_rows_equal(got[:, 32 + i], price[:, src], f"column {32 + i} vs price column {src}")


# --------------------------------------------------------------------------- 5. hw math is f32 only
def test_path_greeks_hw_math_is_f32_only() -> None:
    c = torch.tensor(_contracts(12), dtype=torch.float64, device=DEV)
    out = poisoned((12, COLS), torch.float64, DEV)
    st = _lib.lib().smc_gbm_greeks_paths(_lib.ptr(c), 12, 16, 4096, SEED, None, ORD0, _lib.MATH_HW, 1,
                                         _lib.DTYPE_F64, _lib.ptr(out), None)
    torch.cuda.synchronize()
    assert st == _lib.SMC_ERR_INVALID_ARGUMENT and "f32 only" in _lib.last_error()
    assert bool(torch.isnan(out).all())


# --------------------------------------------------------------------------- 6. degenerate rows
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("norm", [0, 1])
def test_path_greeks_degenerate_contracts(norm, dtype) -> None:
    """v = 0 with mu = 0 (r = d: every row is X0, all rows tie; checked on delta and rho only, as the issue says, plus
    the exact zeros of the v == 0 convention), T = 0 (every row is X0, the cT term is dropped), a single path."""
    c = np.array([[100.0, 95.0, 2.0, 0.03, 0.03, 0.0], [50.0, 40.0, 0.0, 0.1, 0.0, 0.7]])
    eps = 2.0 ** -22 if dtype == 0 else 1e-10
    for T, P in ((8, 256), (5, 2053)):
        got = _greeks(c, T, P, 0, norm, dtype)
        assert not np.isnan(got).any()
        # v = 0, mu = 0: x_t = X0 on every row, so u = X0 > K for all four payoffs: the calls are in the money
        v0 = got[0]
        df = math.exp(-0.03 * 2.0)
        tol = (2 * T + 16) * eps
        for q in (1, 3):  # Asian call, lookback call
            assert abs(v0[0 + q] - df) <= tol, (q, v0[q], df)                     # delta = df u / X0
            # rho = -T df (u - K) + df u mean(tau): the Asian mean of tau is T (steps + 1) / (2 steps), and the
            # lookback's first row wins the tie: tau_0 = T / steps
            tau = 2.0 * (T + 1) / (2 * T) if q == 1 else 2.0 / T
            want = -2.0 * df * 5.0 + df * 100.0 * tau
            assert abs(v0[8 + q] - want) <= tol * 400, (q, v0[8 + q], want)
            assert v0[4 + q] == 0.0 and v0[20 + q] == 0.0                         # vega and its error: v == 0
        for q in (0, 2):  # the puts are never exercised: every column of theirs is exactly 0
            assert np.all(v0[[q, 4 + q, 8 + q, 12 + q, 16 + q, 20 + q, 24 + q, 28 + q, 32 + q, 36 + q]] == 0.0)
        # T = 0: x_t = X0 = 50 > K = 40; df = 1; prices are the intrinsic value exactly; delta = 1; rho = 0 (Tr = tau = 0)
        t0 = got[1]
        for q in (1, 3):
            assert t0[32 + q] == 10.0 and abs(t0[q] - 1.0) <= eps and t0[8 + q] == 0.0
            # theta = r call - df u hT with hT = aT alone: RAW mu / 2 fr_t, NORMALIZE (r - d) fr_t; fr of the Asian
            # average is (steps + 1) / (2 steps), of the lookback's first row 1 / steps
            fr = (T + 1) / (2 * T) if q == 1 else 1.0 / T
            aT = (0.1 - 0.5 * 0.49) / 2.0 * fr if not norm else 0.1 * fr
            assert abs(t0[12 + q] - (0.1 * 10.0 - 50.0 * aT)) <= 64 * eps, (q, t0[12 + q])
        assert np.all(np.abs(t0[STDERR_COLS]) <= 1e-6)
    one = _greeks(_contracts(12), 5, 1, 0, norm, dtype)
    assert not np.isnan(one).any() and np.all(one[:, STDERR_COLS] == 0.0)


# --------------------------------------------------------------------------- 7. Python API
def _engine(dtype: Precision, T: int, N: int, M: int, mc_seed: int = SEED, skip: int = ORD0,
            scheme: PathScheme = PathScheme.LOG_EULER,
            norm: ForwardNormalization = ForwardNormalization.NORMALIZE) -> BlackScholes:
    sp = make_simulation_params(timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=mc_seed, buffer_size=1,
                                skip=skip, dtype=dtype)
    return BlackScholes(make_black_scholes_config(sim_params=sp, path_scheme=scheme, normalization=norm))


def _inputs(c: np.ndarray) -> list[BlackScholes.Inputs]:
    return [BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5]) for r in c.tolist()]


def test_greeks_paths_batch_python_api() -> None:
    c = _contracts(12)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    T, P = 16, 4096
    block = _greeks(c, T, P, 0, 1, 0, ORD0)
    fields = list(BlackScholes.PathBatchGreeks.model_fields)
    assert len(fields) == COLS and fields == list(BlackScholes.HostPathGreeks.model_fields)
    assert fields[0] == "asian_put_delta" and fields[15] == "lookback_call_theta"
    assert fields[31] == "lookback_call_theta_stderr" and fields[32] == "asian_put" and fields[36] == "asian_put_stderr"
    bs = _engine(Precision.float32, T, 64, 64)
    dev = expect_success(bs.greeks_paths_batch_device(cd))
    assert bs.ordinal == ORD0 + 12
    for i, name in enumerate(fields):
        t = getattr(dev, name)
        assert t.shape == (12,) and t.dtype == torch.float64 and t.is_cuda, name
        assert_rows_equal(t.cpu().numpy(), block[:, i], name)
    host_engine = _engine(Precision.float32, T, 64, 64)
    host = expect_success(host_engine.greeks_paths_batch(_inputs(c)))
    assert host_engine.ordinal == ORD0 + 12
    assert len(host) == 12 and all(isinstance(h, BlackScholes.HostPathGreeks) for h in host)
    for i, name in enumerate(fields):
        assert [getattr(h, name) for h in host] == block[:, i].tolist(), name
    assert expect_success(bs.greeks_paths_batch([])) == [] and bs.ordinal == ORD0 + 12
    empty = expect_success(bs.greeks_paths_batch_device(cd[:0]))
    assert all(getattr(empty, name).shape == (0,) for name in fields) and bs.ordinal == ORD0 + 12
    for bad in (cd[:, :5], cd.to(torch.float32), cd.reshape(-1), cd.cpu()):
        with pytest.raises(ValueError):
            bs.greeks_paths_batch_device(bad)
    assert bs.ordinal == ORD0 + 12
    nxt = expect_success(bs.greeks_paths_batch_device(cd[:2]))
    assert_rows_equal(nxt.asian_put_delta.cpu().numpy(), _greeks(c[:2], T, P, 0, 1, 0, ORD0 + 12)[:, 0], "next ordinals")


def test_greeks_paths_batch_rejects_simple_euler_and_hw_f64() -> None:
    bs = _engine(Precision.float32, 16, 64, 64, scheme=PathScheme.SIMPLE_EULER)
    c = _contracts(12)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="SIMPLE_EULER"):
        bs.greeks_paths_batch_device(cd)
    with pytest.raises(ValueError, match="SIMPLE_EULER"):
        bs.greeks_paths_batch(_inputs(c))
    assert bs.ordinal == ORD0
    hw = _engine(Precision.float32, 16, 64, 64)
    hw.price_batch_math = "hw"
    got = expect_success(hw.greeks_paths_batch_device(cd))
    want = _greeks(c, 16, 4096, _lib.MATH_HW, 1, 0, ORD0)
    for i, name in enumerate(BlackScholes.PathBatchGreeks.model_fields):
        assert_rows_equal(getattr(got, name).cpu().numpy(), want[:, i], name)
    raw = _engine(Precision.float64, 16, 64, 64, norm=ForwardNormalization.RAW)
    got = expect_success(raw.greeks_paths_batch_device(cd))
    assert_rows_equal(got.asian_call_vega.cpu().numpy(), _greeks(c, 16, 4096, 0, 0, 1, ORD0)[:, 5], "f64 RAW engine")
    raw.price_batch_math = "hw"
    with pytest.raises(_lib.SmcError) as exc:
        raw.greeks_paths_batch_device(cd)
    assert exc.value.code == _lib.SMC_ERR_INVALID_ARGUMENT and raw.ordinal == ORD0 + 12


def test_greeks_paths_batch_device_is_capturable() -> None:
    c = _contracts(12)
    T, P = 16, 4096
    eager = _greeks(c, T, P, 0, 1, 0, ORD0)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    bs = _engine(Precision.float32, T, 64, 64)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        res = expect_success(bs.greeks_paths_batch_device(cd))
    assert bs.ordinal == ORD0 + 12
    fields = list(BlackScholes.PathBatchGreeks.model_fields)
    for name in fields:  # views of the one block the replay writes: poisoned, so an unwritten element shows
        getattr(res, name).fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(torch.stack([getattr(res, name) for name in fields], dim=1).cpu().numpy(), eager,
                      "replayed graph vs eager")
