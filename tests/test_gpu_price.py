"""Batched Monte-Carlo pricing (smc_gbm_price / BlackScholes.price_batch): the [B][8] block of price_kernel
against the CPU restatement, bit for bit where the kernel promises it (the raw terminal sum, the
intrinsic values, the modes, run to run and under a split of the batch), within stated rounding bounds
elsewhere.

The f32 expectation restates the table of include/spectralmc_hip.h on the oracle's kernel-mode terminal
values (oracle.kernel_paths, wg = 512: the kernel's own streams and terminal-sum order): F, df, K, the
scale s = F / f32(sum / P) and the payoffs in numpy float32 with the portable exp (oracle_exp2), the sums
in float64 (numpy's pairwise order, not the kernel's: hence the P 2^-52 bounds below)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.gbm import BlackScholes
from spectralmc_amd.models.numerical import Precision
from tests.helpers import gbm_restate as gr
from tests.helpers import (
    ATOL_FLOAT64,
    RTOL_FLOAT64,
    assert_rows_equal,
    expect_success,
    make_black_scholes_config,
    make_simulation_params,
    poisoned,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7
COLS = _lib.PRICE_COLS


_contracts = gr.contracts


def _price(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = 0, ordinal0: int = 0,
           seed: int = SEED, ordinal_dev: torch.Tensor | None = None) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_price(_lib.ptr(cd), c.shape[0], T, P, seed, _lib.ptr(ordinal_dev), ordinal0, scheme,
                                        norm, dtype, _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


_stderr = gr.stderr
_block = gr.price_block


@functools.lru_cache(maxsize=None)
def _restated_f32(B: int, T: int, P: int, scheme: int, norm: int, ordinal0: int) -> dict[str, np.ndarray]:
    return gr.price_f32(_oracle, _contracts(B), T, P, SEED, ordinal0, scheme, norm)


def _restated_f64(B: int, T: int, P: int, scheme: int, norm: int, ordinal0: int) -> dict[str, np.ndarray]:
    _oracle.build()
    c = _contracts(B)
    _, term, rs = _oracle.gbm_paths(c, T, P, SEED, ordinal0, scheme, dtype="float64")
    F = c[:, 0] * np.exp((c[:, 3] - c[:, 4]) * c[:, 2])
    df = np.exp(-c[:, 3] * c[:, 2])
    tsum = rs[:, -1].copy()
    s = F / (tsum / P) if norm else np.ones(B)
    return _block(term * s[:, None], c[:, 1].copy(), F, df, tsum)


# (B, T, P, scheme, norm)
F32_CASES = [
    (12, 16, 4096, 0, 1),    # two whole chunks, parked in LDS
    (12, 5, 693, 1, 1),      # simple Euler, odd T, ragged P % 4 != 0
    (12, 3, 2048, 0, 0),     # RAW: one pass
    (12, 1, 528, 0, 1),      # T = 1 (stream span), a partial chunk
    (3, 4, 65536, 0, 1),     # too large to park: replay chosen by the shape
    (600, 3, 2048, 0, 1),    # more contracts than CUs
]
ORD0 = 11


@pytest.mark.parametrize("B,T,P,scheme,norm", F32_CASES)
def test_price_matches_restatement_f32(B, T, P, scheme, norm) -> None:
    want = _restated_f32(B, T, P, scheme, norm, ORD0)
    got = _price(_contracts(B), T, P, scheme, norm, 0, ORD0)
    name = _lib.lib().smc_gbm_price_kernel(T, P, scheme, norm, 0).decode()
    assert name == ("price_kernel(raw)" if not norm else "price_kernel(replay)" if P == 65536 else "price_kernel(lds)")
    w = want["cols"]
    assert not np.isnan(got).any()
    # the raw terminal sum in simulate_contract's order, and the intrinsic values: bit for bit
    assert_rows_equal(got[:, 7], w[:, 7], "terminal sum")
    assert_rows_equal(got[:, 5:7], w[:, 5:7], "intrinsic values")
    # two f64 sums of P non-negative terms in different orders each err by at most (P - 1) 2^-53 relative
    for col in range(3):
        print(f"col {col}: max rel {np.max(np.abs(got[:, col] - w[:, col]) / np.abs(w[:, col])):.3e} (bound {P * 2.0 ** -52:.3e})")
    for col in range(3):
        np.testing.assert_allclose(got[:, col], w[:, col], rtol=P * 2.0 ** -52, atol=0, err_msg=f"col {col}")
    # the standard errors take D = sum v^2 - P m^2: with e = P 2^-52 the bound above, sum v^2 = D + P m^2
    # moves by e (D + P m^2) and P m^2 by 2 e P m^2, so D by e (1 + 3 rho) D with rho = m^2 / var, halved by
    # the square root: below 8 e while rho <= 2 (every contract of the 12-contract cases), and below
    # 8 e (rho / 2) beyond (the 600-contract batch has deep in-the-money calls of rho ~ 10)
    rho = want["m2_over_var"]
    if B <= 12:
        assert float(rho.max()) <= 2.0
    for col in (3, 4):
        tol = 8 * P * 2.0 ** -52 * np.maximum(1.0, rho[:, col - 3] / 2)
        err = np.abs(got[:, col] - w[:, col]) / w[:, col]
        print(f"col {col}: max rel {err.max():.3e}, max share of its bound {np.max(err / tol):.3f}")
        assert np.all(err <= tol), (col, int(np.argmax(err / tol)))
    # what the numbers mean: put-call parity on the same paths, and NORMALIZE puts the mean on the forward
    K = _contracts(B)[:, 1]
    parity = got[:, 1] - got[:, 0] - want["df"] * (got[:, 2] - K)
    assert np.max(np.abs(parity) / K) < 1e-6
    if norm:
        assert np.max(np.abs(got[:, 2] / want["F"] - 1)) < 1e-6


# the largest contracts that are parked: 144 KiB of f32, and the f64 row that fills a CU's 160 KiB of LDS beside
# the table image of the f64 path math (one more path: replay, test_price_host)
MODE_CASES = [(0, 16, 4096), (0, 16, 693), (1, 16, 4096), (1, 16, 693), (0, 2, 36784), (1, 2, 14036)]


@pytest.mark.parametrize("dtype,T,P", MODE_CASES)
def test_price_modes_agree_bitwise(dtype, T, P) -> None:
    """Parked in LDS and replayed: the same values in the same order (f32 at the issue's shape; f64, a
    ragged P and the largest parked rows as well)."""
    c = _contracts(12)
    L = _lib.lib()
    assert L.smc_gbm_price_kernel(T, P, 0, 1, dtype) == b"price_kernel(lds)"
    assert L.smc_gbm_price_kernel(T, P + 1, 0, 1, dtype) == (b"price_kernel(replay)" if P > 4096 else b"price_kernel(lds)")
    assert L.smc_gbm_price_kernel(T, P, _lib.PRICE_REPLAY, 1, dtype) == b"price_kernel(replay)"
    lds = _price(c, T, P, 0, 1, dtype, ORD0)
    replay = _price(c, T, P, _lib.PRICE_REPLAY, 1, dtype, ORD0)
    assert not np.isnan(lds).any()
    assert_rows_equal(replay, lds, "replay vs lds")
    if P > 4096:  # the parked row's far end holds what the streams give: the sum over all P paths
        _oracle.build()
        _, _, rs = _oracle.kernel_paths(c, T, P, SEED, ORD0, 0) if dtype == 0 else \
            _oracle.gbm_paths(c, T, P, SEED, ORD0, 0, dtype="float64")
        np.testing.assert_allclose(lds[:, 7], rs[:, -1], rtol=0 if dtype == 0 else 5e-11, atol=0)
        assert np.max(np.abs(lds[:, 2] / (c[:, 0] * np.exp((c[:, 3] - c[:, 4]) * c[:, 2])) - 1)) < 1e-6


def test_price_is_deterministic_and_splits() -> None:
    c = _contracts(12)
    T, P = 16, 4096
    whole = _price(c, T, P, 0, 1, 0, 100)
    assert_rows_equal(_price(c, T, P, 0, 1, 0, 100), whole, "run to run")
    assert_rows_equal(_price(c[5:], T, P, 0, 1, 0, 105), whole[5:], "batch split at contract 5")
    # the same with the ordinal's offset on the device, all of it and part of it
    for dev_part in (105, 40):
        od = torch.tensor([dev_part], dtype=torch.int64, device=DEV)
        assert_rows_equal(_price(c[5:], T, P, 0, 1, 0, 105 - dev_part, ordinal_dev=od), whole[5:],
                          f"ordinal_dev = {dev_part}")
    # other ordinals are other streams
    assert not np.array_equal(_price(c, T, P, 0, 1, 0, 101)[:, 7], whole[:, 7])


@pytest.mark.parametrize("B,T,P,scheme,norm", [(6, 16, 4096, 0, 1), (6, 7, 1024, 1, 0)])
def test_price_matches_oracle_f64(B, T, P, scheme, norm) -> None:
    want = _restated_f64(B, T, P, scheme, norm, ORD0)
    got = _price(_contracts(B), T, P, scheme, norm, 1, ORD0)
    w = want["cols"]
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got[:, 7], w[:, 7], rtol=5e-11, atol=0)    # as test_paths_match_oracle's row sums
    np.testing.assert_allclose(got[:, :3], w[:, :3], rtol=1e-10, atol=0)  # the project's f64 tolerance
    np.testing.assert_allclose(got[:, 5:7], w[:, 5:7], rtol=1e-10, atol=0)
    for col in (3, 4):
        tol = 1e-10 * (1 + 2 * want["m2_over_var"][:, col - 3])
        assert np.all(np.abs(got[:, col] - w[:, col]) <= tol * np.abs(w[:, col])), col


def test_price_hw_math_close_to_portable() -> None:
    B, T, P = 32, 16, 4096
    want = _restated_f32(B, T, P, 0, 1, ORD0)["cols"]
    got = _price(_contracts(B), T, P, _lib.MATH_HW, 1, 0, ORD0)
    assert not np.isnan(got).any()
    for col in range(3):  # batch norm-relative, the project's 1e-5 for hardware-transcendental f32 runs
        rel = float(np.linalg.norm(got[:, col] - want[:, col]) / np.linalg.norm(want[:, col]))
        print(f"col {col}: batch norm-relative {rel:.3e}")
        assert rel < 1e-5, col
    assert_rows_equal(got[:, 5:7], want[:, 5:7], "intrinsic values do not use the path math")


@pytest.mark.parametrize("dtype", [0, 1])
def test_price_degenerate_contracts(dtype) -> None:
    """v = 0 and T = 0 (test_zero_vol_and_zero_maturity_exact's rows): every path ends on the forward, so
    the prices are the intrinsic values.  Under NORMALIZE xs = x (F / mean x) with mean x = x exactly: three
    roundings of the sim dtype (quotient, product, difference), below 2^-22 of the contract's scale max(K, F)."""
    c = np.array([[100.0, 95.0, 2.0, 0.05, 0.01, 0.0], [50.0, 40.0, 0.0, 0.1, 0.0, 0.7],
                  [100.0, 120.0, 2.0, 0.05, 0.01, 0.0]])
    for T, P in ((8, 256), (3, 2053)):
        for flag in (0, _lib.PRICE_REPLAY):
            got = _price(c, T, P, flag, 1, dtype)
            assert not np.isnan(got).any()
            F = c[:, 0] * np.exp((c[:, 3] - c[:, 4]) * c[:, 2])
            scale = np.maximum(c[:, 1], F)
            assert np.all(np.abs(got[:, 0] - got[:, 5]) <= 2.0 ** -22 * scale)
            assert np.all(np.abs(got[:, 1] - got[:, 6]) <= 2.0 ** -22 * scale)
            assert np.all(got[:, 3:5] <= 1e-6 * c[:, 1:2])
            assert got[1, 5] == 0.0 and got[1, 6] == 10.0 and got[1, 7] == 50.0 * P  # T = 0: exact
            assert got[0, 5] == 0.0 and got[2, 6] == 0.0 and got[0, 6] > 0 and got[2, 5] > 0


def test_price_single_path_has_zero_stderr() -> None:
    got = _price(_contracts(12), 4, 1, 0, 1, 0)
    assert not np.isnan(got).any()
    assert np.all(got[:, 3:5] == 0.0)


def _engine(dtype: Precision, T: int, N: int, M: int, mc_seed: int = 19, skip: int = 0) -> BlackScholes:
    sp = make_simulation_params(timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=mc_seed, buffer_size=1,
                                skip=skip, dtype=dtype)
    return BlackScholes(make_black_scholes_config(sim_params=sp))


def _inputs(c: np.ndarray) -> list[BlackScholes.Inputs]:
    return [BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5]) for r in c.tolist()]


def test_price_batch_python_api() -> None:
    batch, loop = _engine(Precision.float64, 8, 64, 64, skip=3), _engine(Precision.float64, 8, 64, 64, skip=3)
    cs = _inputs(_contracts(12))
    assert expect_success(batch.price_batch([])) == [] and batch.ordinal == 3
    got = expect_success(batch.price_batch(cs))
    want = [expect_success(loop.price_to_host(c)) for c in cs]
    assert len(got) == len(cs) and all(isinstance(g, BlackScholes.HostPricingResults) for g in got)
    for name in ("put_price", "call_price", "underlying", "put_price_intrinsic", "call_price_intrinsic"):
        np.testing.assert_allclose([getattr(g, name) for g in got], [getattr(w, name) for w in want],
                                   rtol=RTOL_FLOAT64, atol=ATOL_FLOAT64, err_msg=name)
    for g in got:
        assert g.put_convexity == g.put_price - g.put_price_intrinsic
        assert g.call_convexity == g.call_price - g.call_price_intrinsic
        assert min(g.put_price_intrinsic, g.call_price_intrinsic) == 0.0
    # both consumed len(cs) normal streams, and go on alike
    for eng in (batch, loop):
        assert expect_success(eng.snapshot()).sim_params.skip == 3 + len(cs)
    nxt_b, nxt_l = expect_success(batch.price_to_host(cs[0])), expect_success(loop.price_to_host(cs[0]))
    assert nxt_b == nxt_l
    # the device form: [B] f64 tensors on the device, the same launch
    fresh = _engine(Precision.float64, 8, 64, 64, skip=3)
    cd = torch.tensor(_contracts(12), dtype=torch.float64, device=DEV)
    dev = expect_success(fresh.price_batch_device(cd))
    assert fresh.ordinal == 3 + len(cs)
    for name in BlackScholes.BatchPrices.model_fields:
        t = getattr(dev, name)
        assert t.shape == (len(cs),) and t.dtype == torch.float64 and t.is_cuda, name
    assert dev.put_price.cpu().tolist() == [g.put_price for g in got]
    assert dev.call_price.cpu().tolist() == [g.call_price for g in got]
    assert float(dev.put_stderr.min()) > 0 and float(dev.terminal_sum.min()) > 0
    empty = expect_success(fresh.price_batch_device(cd[:0]))
    assert empty.put_price.shape == (0,) and fresh.ordinal == 3 + len(cs)
    # hardware math is a float32 mode: the f64 engine reports the C ABI's status
    fresh.price_batch_math = "hw"
    with pytest.raises(_lib.SmcError) as exc:
        fresh.price_batch_device(cd)
    assert exc.value.code == _lib.SMC_ERR_INVALID_ARGUMENT and fresh.ordinal == 3 + len(cs)


def test_price_batch_hw_math_f32_engine() -> None:
    """price_batch_math = "hw" on a float32 engine: the SMC_MATH_HW launch (bit for bit the C call's), within
    the f32 batch tolerance of the portable default."""
    c = _contracts(32)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    hw, portable = _engine(Precision.float32, 16, 64, 64, mc_seed=SEED, skip=ORD0), \
        _engine(Precision.float32, 16, 64, 64, mc_seed=SEED, skip=ORD0)
    hw.price_batch_math = "hw"
    got, ref = expect_success(hw.price_batch_device(cd)), expect_success(portable.price_batch_device(cd))
    assert got.put_price.cpu().tolist() == _price(c, 16, 4096, _lib.MATH_HW, 1, 0, ORD0)[:, 0].tolist()
    assert ref.put_price.cpu().tolist() == _price(c, 16, 4096, 0, 1, 0, ORD0)[:, 0].tolist()
    assert float((got.put_price - ref.put_price).norm() / ref.put_price.norm()) < 1e-5


def test_price_batch_reports_an_invalid_normal_buffer() -> None:
    from spectralmc_amd.errors.gbm import NormalsUnavailable
    from spectralmc_amd.result import Failure

    sp = make_simulation_params(timesteps=2, network_size=4, batches_per_mc_run=2, buffer_size=1000)
    bs = BlackScholes(make_black_scholes_config(sim_params=sp))
    cs = _inputs(_contracts(12))[:2]
    one = bs.price_to_host(cs[0])
    cd = torch.tensor(_contracts(12)[:2], dtype=torch.float64, device=DEV)
    for res in (bs.price_batch(cs), bs.price_batch([]), bs.price_batch_device(cd)):
        assert isinstance(res, Failure) and isinstance(res.error, NormalsUnavailable)
        assert res.error == one.error
    assert bs.ordinal == 0


def test_price_against_the_closed_form(oracle) -> None:
    """64 contracts, one exact log-Euler step, 262,144 paths each (the replay mode): the bar of
    test_gbm_engine_price_vs_black on the relative error, and every put within 5 of its own standard errors
    (the CPU restatement of these draws: worst 2.58 standard errors, RMSPE 1.8e-3)."""
    c = _contracts(64)
    got = _price(c, 1, 256 * 1024, 0, 1, 0, ordinal0=5, seed=31)
    assert not np.isnan(got).any()
    black = np.array([oracle.black_put(*row) for row in c.tolist()])
    z = np.abs(got[:, 0] - black) / got[:, 3]
    rmspe = float(np.sqrt(np.mean(np.square((got[:, 0] - black) / black))))
    print(f"rmspe {rmspe:.3e}, worst |put - black| / stderr {z.max():.2f}")
    assert rmspe < 0.02
    assert np.all(z <= 5.0)


def test_price_call_is_capturable() -> None:
    c = _contracts(12)
    T, P = 16, 4096
    eager = _price(c, T, P, 0, 1, 0, ORD0)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((12, COLS), torch.float64, DEV)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        _lib.check(_lib.lib().smc_gbm_price(_lib.ptr(cd), 12, T, P, SEED, None, ORD0, 0, 1, 0, _lib.ptr(out),
                                            _lib.stream_handle()))
    assert bool(torch.isnan(out).all())  # capturing launches nothing
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(out.cpu().numpy(), eager, "replayed graph vs eager")
