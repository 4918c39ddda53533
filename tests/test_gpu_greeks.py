"""Batched pathwise Greeks (smc_gbm_greeks / BlackScholes.greeks_batch): the [B][26] block of greeks_kernel
against the CPU restatement of the table in include/spectralmc_hip.h (tests/helpers/greeks_restate.py), bit for
bit where the kernel promises it (the raw terminal sum, the price call's columns, the modes, run to run and under a split of the batch), within
stated rounding bounds elsewhere, and against the Black-Scholes closed forms within the Monte-Carlo error.

The f32 expectation follows the header's formulas operation by operation in numpy float32 on the oracle's
kernel-mode terminal values (oracle.kernel_paths, wg = 512: the kernel's own streams and terminal-sum order),
with the portable exp (oracle_exp2) and log (oracle_log_pos); the sums are float64 in numpy's pairwise order,
not the kernel's: hence the P 2^-52 bounds below."""

from __future__ import annotations

import functools
import math

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
from tests.helpers.greeks_restate import check_stderr as _check_stderr
from tests.helpers.greeks_restate import log_pos_f32 as _log_pos_f32
from tests.helpers.greeks_restate import summary as _summary
from tests.helpers.greeks_restate import terms as _terms

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7
ORD0 = 11
COLS = _lib.GREEKS_COLS
MEANS = list(range(10))
NAMES = ["put_delta", "call_delta", "put_vega", "call_vega", "put_rho", "call_rho", "put_theta", "call_theta",
         "put_gamma", "call_gamma"]


@functools.lru_cache(maxsize=None)
def _contracts(n: int) -> np.ndarray:
    """tests/test_gpu_price.py's generator."""
    rng = np.random.default_rng(2026)
    rows = []
    for _ in range(n):
        x0 = rng.uniform(50, 150)
        k = x0 * rng.uniform(0.8, 1.25)
        rows.append([x0, k, rng.uniform(0.25, 2), rng.uniform(-0.02, 0.08), rng.uniform(0, 0.04),
                     rng.uniform(0.1, 0.6)])
    out = np.array(rows, dtype=np.float64)
    out.setflags(write=False)
    return out


def _call(fn, cols: int, c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int, ordinal0: int,
          seed: int, ordinal_dev: torch.Tensor | None) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], cols), torch.float64, DEV)
    _lib.check(fn(_lib.ptr(cd), c.shape[0], T, P, seed, _lib.ptr(ordinal_dev), ordinal0, scheme, norm, dtype,
                  _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _greeks(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = 0, ordinal0: int = ORD0,
            seed: int = SEED, ordinal_dev: torch.Tensor | None = None) -> np.ndarray:
    return _call(_lib.lib().smc_gbm_greeks, COLS, c, T, P, scheme, norm, dtype, ordinal0, seed, ordinal_dev)


def _price(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = 0, ordinal0: int = ORD0,
           seed: int = SEED) -> np.ndarray:
    return _call(_lib.lib().smc_gbm_price, _lib.PRICE_COLS, c, T, P, scheme, norm, dtype, ordinal0, seed, None)


def _name(T: int, P: int, scheme: int, norm: int, dtype: int = 0) -> str:
    return _lib.lib().smc_gbm_greeks_kernel(T, P, scheme, norm, dtype).decode()


@functools.lru_cache(maxsize=None)
def _paths_f32(B: int, T: int, P: int, ordinal0: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(terminal values [B,P] f32, their portable logs L = log_pos(x / f32(X0)), the oracle's terminal sums)."""
    _oracle.build()
    c = _contracts(B)
    _, term, rs = _oracle.kernel_paths(c, T, P, SEED, ordinal0, 0)
    L = _log_pos_f32(term / c[:, 0].astype(np.float32)[:, None])
    for a in (term, L):
        a.setflags(write=False)
    return term, L, rs[:, -1].copy()


# --------------------------------------------------------------------------- 1. restatement, portable f32
# (B, T, P, norm)
F32_CASES = [
    (12, 16, 4096, 1),    # two whole chunks, parked in LDS
    (12, 5, 693, 1),      # odd T, ragged P % 4 != 0
    (12, 3, 2048, 0),     # RAW: one pass
    (12, 1, 528, 1),      # T = 1 (stream span), a partial chunk
    (3, 4, 65536, 1),     # too large to park: replay chosen by the shape
    (300, 3, 1024, 1),    # more contracts than CUs
]


@pytest.mark.parametrize("B,T,P,norm", F32_CASES)
def test_greeks_match_restatement_f32(B, T, P, norm) -> None:
    c = _contracts(B)
    term, L, tsum = _paths_f32(B, T, P, ORD0)
    got = _greeks(c, T, P, 0, norm, 0, ORD0)
    assert _name(T, P, 0, norm) == ("greeks_kernel(raw)" if not norm else
                                    "greeks_kernel(replay)" if P == 65536 else "greeks_kernel(lds)")
    assert not np.isnan(got).any()
    # the raw terminal sum in simulate_contract's order: bit for bit
    assert_rows_equal(got[:, 24], tsum, "terminal sum")
    xl = (term * L).astype(np.float64)
    if norm:
        want_xl, bound_xl = xl.sum(axis=1), P * 2.0 ** -52 * np.abs(xl).sum(axis=1)
        print(f"sumxl: max share of its bound {np.max(np.abs(got[:, 25] - want_xl) / bound_xl):.3e}")
        assert np.all(np.abs(got[:, 25] - want_xl) <= bound_xl)
    else:
        assert np.all(got[:, 25] == 0.0)
    # Lbar from the kernel's own columns 24 and 25: Real(av) and Real(aT) are roundings of functions of it, and a
    # one-ulp move of either (which a sum-order difference in column 25 can cause) would move every path's term
    r = _terms(c, term, norm, got[:, 24], got[:, 25], L)
    s = _summary(r["t"], c)
    w = s["cols"]
    # two f64 sums of the same P terms in different orders differ by at most P 2^-52 sum|term|, here over P
    for col in MEANS:
        err, bound = np.abs(got[:, col] - w[:, col]), s["bound"][col]
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0, 0.0, err / bound)
        print(f"{NAMES[col]}: max share of its bound {share.max():.3e}")
        assert np.all(err <= bound), (NAMES[col], int(np.argmax(share)))
    for i, col in enumerate((20, 21)):
        assert np.all(np.abs(got[:, col] - w[:, col]) <= s["price_bound"][i]), col
    den = c[:, 5] * c[:, 2] * c[:, 0] * c[:, 0]
    for term_i in range(8):
        _check_stderr(got[:, 10 + term_i], w[:, 10 + term_i], s, term_i, P, NAMES[term_i])
    for i in range(2):  # gamma's error is vega's over v T X0^2, the prices' are columns 22, 23
        _check_stderr(got[:, 18 + i], w[:, 18 + i], s, 2 + i, P, NAMES[8 + i], scale=1.0 / den)
        _check_stderr(got[:, 22 + i], w[:, 22 + i], s, 8 + i, P, ("put", "call")[i])


# --------------------------------------------------------------------------- 2. ties to the price call
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("T,P", [(16, 4096), (5, 693)])
def test_greeks_price_columns_are_the_price_call(T, P, norm, dtype) -> None:
    c = _contracts(12)
    got = _greeks(c, T, P, 0, norm, dtype)
    price = _price(c, T, P, 0, norm, dtype)
    assert not np.isnan(got).any() and not np.isnan(price).any()
    assert_rows_equal(got[:, 20:25], price[:, [0, 1, 3, 4, 7]], "columns 20..24 vs smc_gbm_price 0, 1, 3, 4, 7")


# --------------------------------------------------------------------------- 3. modes
# the large P lie just under the switch points test_greeks_host finds (36,784 f32, 14,036 f64)
MODE_CASES = [(0, 16, 4096), (0, 16, 693), (0, 2, 36000), (1, 16, 4096), (1, 2, 14000)]


@pytest.mark.parametrize("dtype,T,P", MODE_CASES)
def test_greeks_modes_agree_bitwise(dtype, T, P) -> None:
    c = _contracts(12)
    assert _name(T, P, 0, 1, dtype) == "greeks_kernel(lds)"
    assert _name(T, P, _lib.PRICE_REPLAY, 1, dtype) == "greeks_kernel(replay)"
    lds = _greeks(c, T, P, 0, 1, dtype)
    replay = _greeks(c, T, P, _lib.PRICE_REPLAY, 1, dtype)
    assert not np.isnan(lds).any()
    assert_rows_equal(replay, lds, "replay vs lds")
    if P > 4096:  # the parked row's far end holds what the streams give: the price call's sum over all P paths
        assert_rows_equal(lds[:, 24], _price(c, T, P, _lib.PRICE_REPLAY, 1, dtype)[:, 7], "terminal sum")


# --------------------------------------------------------------------------- 4. determinism and splitting
def test_greeks_are_deterministic_and_split() -> None:
    c = _contracts(12)
    T, P = 16, 4096
    whole = _greeks(c, T, P, 0, 1, 0, 100)
    assert not np.isnan(whole).any()
    assert_rows_equal(_greeks(c, T, P, 0, 1, 0, 100), whole, "run to run")
    assert_rows_equal(_greeks(c[5:], T, P, 0, 1, 0, 105), whole[5:], "batch split at contract 5")
    assert_rows_equal(_greeks(c[:5], T, P, 0, 1, 0, 100), whole[:5], "batch split at contract 5, the head")
    for dev_part in (105, 40):
        od = torch.tensor([dev_part], dtype=torch.int64, device=DEV)
        assert_rows_equal(_greeks(c[5:], T, P, 0, 1, 0, 105 - dev_part, ordinal_dev=od), whole[5:],
                          f"ordinal_dev = {dev_part}")
    assert not np.array_equal(_greeks(c, T, P, 0, 1, 0, 101)[:, 24], whole[:, 24])  # other ordinals, other streams


# --------------------------------------------------------------------------- 5. closed form
def _ncdf(x: float) -> float:
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def _black_scholes_greeks(X0: float, K: float, T: float, r: float, d: float, v: float) -> list[float]:
    """Columns 0..9 for a European put / call with continuous dividend yield d; theta is -dV/dT per year."""
    sq = v * math.sqrt(T)
    d1 = (math.log(X0 / K) + (r - d + 0.5 * v * v) * T) / sq
    d2 = d1 - sq
    pdf = math.exp(-0.5 * d1 * d1) / math.sqrt(2.0 * math.pi)
    eq, er = math.exp(-d * T), math.exp(-r * T)
    vega = X0 * eq * pdf * math.sqrt(T)
    decay = -X0 * eq * pdf * v / (2.0 * math.sqrt(T))
    gamma = eq * pdf / (X0 * sq)
    return [-eq * _ncdf(-d1), eq * _ncdf(d1), vega, vega, -K * T * er * _ncdf(-d2), K * T * er * _ncdf(d2),
            decay + r * K * er * _ncdf(-d2) - d * X0 * eq * _ncdf(-d1),
            decay - r * K * er * _ncdf(d2) + d * X0 * eq * _ncdf(d1), gamma, gamma]


@pytest.mark.parametrize("norm", [0, 1])
def test_greeks_against_the_closed_form(norm) -> None:
    """Every Greek within 4 of its own standard errors of the Black-Scholes value (the CPU restatement of these
    draws alone stays within 2.21: the cap is a condition, not a measurement), and the identities that hold on
    the paths themselves."""
    B, T, P = 12, 16, 4096
    c = _contracts(B)
    got = _greeks(c, T, P, 0, norm, 0, ORD0)
    assert not np.isnan(got).any()
    black = np.array([_black_scholes_greeks(*row) for row in c.tolist()])
    z = np.abs(got[:, :10] - black) / got[:, 10:20]
    for col in MEANS:
        print(f"{NAMES[col]}: worst |mc - closed form| / stderr {z[:, col].max():.2f}")
    assert np.all(z <= 4.0), np.argwhere(z > 4.0).tolist()
    if norm:
        # NORMALIZE puts the mean of xs on the forward, so call delta - put delta = df F / X0 = e^{-dT}, and its
        # weights L - Lbar have x-weighted mean zero, so the two vegas are the same number
        assert np.max(np.abs(got[:, 1] - got[:, 0] - np.exp(-c[:, 4] * c[:, 2]))) < 1e-5
        assert np.all(np.abs(got[:, 3] - got[:, 2]) <= 1e-5 * (np.abs(got[:, 3]) + np.abs(got[:, 2])))
    # call rho - put rho = T K df (1 - share of paths with xs == K), to the two columns' sum-order bounds
    term, L, _ = _paths_f32(B, T, P, ORD0)
    r = _terms(c, term, norm, got[:, 24], got[:, 25], L)
    s = _summary(r["t"], c)
    exercised = ((r["xs"] != r["K"][:, None]).sum(axis=1)).astype(np.float64)
    want = r["crho"] * exercised / P
    assert np.all(np.abs(got[:, 5] - got[:, 4] - want) <= s["bound"][4] + s["bound"][5] + 2.0 ** -52 * want)
    np.testing.assert_allclose(r["crho"], c[:, 2] * c[:, 1] * np.exp(-c[:, 3] * c[:, 2]), rtol=1e-6)


# --------------------------------------------------------------------------- 6. f64
@pytest.mark.parametrize("B,T,P,norm", [(12, 16, 4096, 1), (12, 3, 2048, 0)])
def test_greeks_match_oracle_f64(B, T, P, norm) -> None:
    """The same formulas in numpy float64 on the oracle's f64 paths, numpy's log, Lbar from numpy's own sums, at
    the project's f64 tolerance.  The library log needs no allowance: measured on an MI355X, the largest error of
    any mean or price column is 3.8e-5 of that tolerance, of vega and theta 1.0e-5 (profiles/greeks/)."""
    _oracle.build()
    c = _contracts(B)
    _, term, rs = _oracle.gbm_paths(c, T, P, SEED, ORD0, 0, dtype="float64")
    L = np.log(term / c[:, 0][:, None])
    sumx = rs[:, -1].copy()
    sumxl = (term * L).sum(axis=1)
    s = _summary(_terms(c, term, norm, sumx, sumxl, L)["t"], c)
    w = s["cols"]
    got = _greeks(c, T, P, 0, norm, 1, ORD0)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got[:, 24], sumx, rtol=5e-11, atol=0)   # as test_price_matches_oracle_f64
    if norm:
        np.testing.assert_allclose(got[:, 25], sumxl, rtol=RTOL_FLOAT64, atol=ATOL_FLOAT64)
    else:
        assert np.all(got[:, 25] == 0.0)
    for col in MEANS + [20, 21]:
        name = NAMES[col] if col < 10 else ("put", "call")[col - 20]
        err = np.abs(got[:, col] - w[:, col])
        print(f"{name}: max |err| / (atol + rtol |want|) {np.max(err / (ATOL_FLOAT64 + RTOL_FLOAT64 * np.abs(w[:, col]))):.3e}")
    for col in MEANS + [20, 21]:
        np.testing.assert_allclose(got[:, col], w[:, col], rtol=RTOL_FLOAT64, atol=ATOL_FLOAT64, err_msg=str(col))
    # the standard errors as test_price_matches_oracle_f64 takes them: 1e-10 (1 + 2 rho)
    pairs = [(10 + i, i) for i in range(8)] + [(18, 2), (19, 3), (22, 8), (23, 9)]
    for col, term_i in pairs:
        assert np.all(np.isfinite(s["rho"][term_i]))  # every contract has paths on both sides of the strike
        tol = RTOL_FLOAT64 * (1 + 2 * s["rho"][term_i]) * np.abs(w[:, col]) + ATOL_FLOAT64
        assert np.all(np.abs(got[:, col] - w[:, col]) <= tol), col


# --------------------------------------------------------------------------- 7. hardware math
@pytest.mark.parametrize("norm", [0, 1])
def test_greeks_hw_math_close_to_portable(norm) -> None:
    """The same uniforms, so the two runs differ by rounding and by at most a path or two whose indicator flips
    at the strike (one flip is about 1 / sqrt(P) = 0.016 standard errors)."""
    c = _contracts(12)
    T, P = 16, 4096
    portable = _greeks(c, T, P, 0, norm, 0)
    hw = _greeks(c, T, P, _lib.MATH_HW, norm, 0)
    assert not np.isnan(hw).any()
    share = np.abs(hw[:, :10] - portable[:, :10]) / portable[:, 10:20]
    print(f"largest |hw - portable| / stderr: {share.max():.4f} ({NAMES[int(np.argmax(share.max(axis=0)))]})")
    assert np.all(share <= 0.1), np.argwhere(share > 0.1).tolist()


def test_greeks_hw_math_is_f32_only() -> None:
    c = torch.tensor(_contracts(12), dtype=torch.float64, device=DEV)
    out = poisoned((12, COLS), torch.float64, DEV)
    st = _lib.lib().smc_gbm_greeks(_lib.ptr(c), 12, 16, 4096, SEED, None, ORD0, _lib.MATH_HW, 1, _lib.DTYPE_F64,
                                   _lib.ptr(out), None)
    torch.cuda.synchronize()
    assert st == _lib.SMC_ERR_INVALID_ARGUMENT and "f32 only" in _lib.last_error()
    assert bool(torch.isnan(out).all())


# --------------------------------------------------------------------------- 8. degenerate contracts
PUT_COLS = [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22]
CALL_COLS = [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23]
STDERR_COLS = list(range(10, 20)) + [22, 23]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("norm", [0, 1])
def test_greeks_degenerate_contracts(norm, dtype) -> None:
    """One batch: v = 0 (every path ends on the forward, in the money for the call), T = 0 (x = X0, in the money
    for the call), a put and a call that no path exercises."""
    c = np.array([[100.0, 95.0, 2.0, 0.05, 0.01, 0.0], [50.0, 40.0, 0.0, 0.1, 0.0, 0.7],
                  [100.0, 20.0, 1.0, 0.03, 0.0, 0.2], [100.0, 1000.0, 1.0, 0.03, 0.0, 0.2]])
    eps = 2.0 ** -22 if dtype == 0 else 1e-10
    for T, P in ((8, 256), (3, 2053)):
        got = _greeks(c, T, P, 0, norm, dtype)
        assert not np.isnan(got).any()
        # v = 0: vega, gamma and their errors are exactly 0; the call's delta is df xs / X0 = e^{-dT}, the put's 0
        v0 = got[0]
        assert np.all(v0[[2, 3, 8, 9, 12, 13, 18, 19]] == 0.0)
        assert np.all(v0[PUT_COLS] == 0.0)
        # (RAW: each of the T steps rounds the path and carries the exp's 0.64 ulp, 2 ulp a step at the most)
        steps = (2 * T + 8) * eps / 2
        assert abs(v0[1] - math.exp(-0.01 * 2.0)) <= steps and abs(v0[11]) <= 1e-6
        assert abs(v0[5] - 2.0 * 95.0 * math.exp(-0.1)) <= 4 * eps * 190 and abs(v0[15]) <= 1e-6 * 190
        # T = 0: gamma is 0 and theta's L / (2 T) part is dropped, so hT = aT (under NORMALIZE r - d, which makes
        # the call's theta the limit d X0 - r K of -dV/dT in the money); the prices are the intrinsic values, exactly
        t0 = got[1]
        assert np.all(t0[[8, 9, 18, 19]] == 0.0) and np.all(t0[PUT_COLS] == 0.0)
        assert t0[20] == 0.0 and t0[21] == 10.0 and t0[24] == 50.0 * P
        assert abs(t0[1] - 1.0) <= eps and t0[5] == 0.0
        want_theta = 0.1 * 10.0 - 50.0 * ((0.1 - 0.5 * 0.49) / 2.0 if not norm else 0.1)
        assert abs(t0[7] - want_theta) <= 64 * eps, (t0[7], want_theta)
        assert np.all(np.abs(t0[STDERR_COLS]) <= 1e-6)
        # nothing exercised: every column of that side is exactly 0
        assert np.all(got[2][PUT_COLS] == 0.0) and got[2][21] > 0
        assert np.all(got[3][CALL_COLS] == 0.0) and got[3][20] > 0


@pytest.mark.parametrize("norm", [0, 1])
def test_greeks_single_path_has_zero_stderr(norm) -> None:
    got = _greeks(_contracts(12), 4, 1, 0, norm, 0)
    assert not np.isnan(got).any()
    assert np.all(got[:, STDERR_COLS] == 0.0)


# --------------------------------------------------------------------------- 9. Python API
def _engine(dtype: Precision, T: int, N: int, M: int, mc_seed: int = SEED, skip: int = ORD0,
            scheme: PathScheme = PathScheme.LOG_EULER,
            norm: ForwardNormalization = ForwardNormalization.NORMALIZE) -> BlackScholes:
    sp = make_simulation_params(timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=mc_seed, buffer_size=1,
                                skip=skip, dtype=dtype)
    return BlackScholes(make_black_scholes_config(sim_params=sp, path_scheme=scheme, normalization=norm))


def _inputs(c: np.ndarray) -> list[BlackScholes.Inputs]:
    return [BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5]) for r in c.tolist()]


def test_greeks_batch_python_api() -> None:
    c = _contracts(12)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    T, P = 16, 4096
    block = _greeks(c, T, P, 0, 1, 0, ORD0)
    fields = list(BlackScholes.BatchGreeks.model_fields)
    assert len(fields) == COLS
    # the device form: the C call's block column by column, and the ordinal moves on by B
    bs = _engine(Precision.float32, T, 64, 64)
    dev = expect_success(bs.greeks_batch_device(cd))
    assert bs.ordinal == ORD0 + 12
    for i, name in enumerate(fields):
        t = getattr(dev, name)
        assert t.shape == (12,) and t.dtype == torch.float64 and t.is_cuda, name
        assert_rows_equal(t.cpu().numpy(), block[:, i], name)
    # the host form: one HostGreeks per contract, the same numbers
    host_engine = _engine(Precision.float32, T, 64, 64)
    host = expect_success(host_engine.greeks_batch(_inputs(c)))
    assert host_engine.ordinal == ORD0 + 12
    assert len(host) == 12 and all(isinstance(h, BlackScholes.HostGreeks) for h in host)
    for i, name in enumerate(fields):
        assert [getattr(h, name) for h in host] == block[:, i].tolist(), name
    # empty inputs: empty results, no launch, the ordinal stays
    assert expect_success(bs.greeks_batch([])) == [] and bs.ordinal == ORD0 + 12
    empty = expect_success(bs.greeks_batch_device(cd[:0]))
    assert all(getattr(empty, name).shape == (0,) for name in fields) and bs.ordinal == ORD0 + 12
    # the price call's tensor validation
    for bad in (cd[:, :5], cd.to(torch.float32), cd.reshape(-1), cd.cpu()):
        with pytest.raises(ValueError):
            bs.greeks_batch_device(bad)
    assert bs.ordinal == ORD0 + 12
    # the next batch goes on where the price call would
    nxt = expect_success(bs.greeks_batch_device(cd[:2]))
    assert_rows_equal(nxt.put_delta.cpu().numpy(), _greeks(c[:2], T, P, 0, 1, 0, ORD0 + 12)[:, 0], "next ordinals")


def test_greeks_batch_rejects_simple_euler() -> None:
    bs = _engine(Precision.float32, 16, 64, 64, scheme=PathScheme.SIMPLE_EULER)
    cd = torch.tensor(_contracts(12), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="SIMPLE_EULER"):
        bs.greeks_batch_device(cd)
    with pytest.raises(ValueError, match="SIMPLE_EULER"):
        bs.greeks_batch(_inputs(_contracts(12)))
    assert bs.ordinal == ORD0


def test_greeks_batch_hw_math_and_raw_engine() -> None:
    c = _contracts(12)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    hw = _engine(Precision.float32, 16, 64, 64)
    hw.price_batch_math = "hw"
    got = expect_success(hw.greeks_batch_device(cd))
    want = _greeks(c, 16, 4096, _lib.MATH_HW, 1, 0, ORD0)
    for i, name in enumerate(BlackScholes.BatchGreeks.model_fields):
        assert_rows_equal(getattr(got, name).cpu().numpy(), want[:, i], name)
    raw = _engine(Precision.float64, 16, 64, 64, norm=ForwardNormalization.RAW)
    got = expect_success(raw.greeks_batch_device(cd))
    assert_rows_equal(got.call_vega.cpu().numpy(), _greeks(c, 16, 4096, 0, 0, 1, ORD0)[:, 3], "f64 RAW engine")
    # hardware math is a float32 mode: the f64 engine reports the C ABI's status and consumes nothing
    raw.price_batch_math = "hw"
    with pytest.raises(_lib.SmcError) as exc:
        raw.greeks_batch_device(cd)
    assert exc.value.code == _lib.SMC_ERR_INVALID_ARGUMENT and raw.ordinal == ORD0 + 12


def test_greeks_batch_device_is_capturable() -> None:
    c = _contracts(12)
    T, P = 16, 4096
    eager = _greeks(c, T, P, 0, 1, 0, ORD0)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    bs = _engine(Precision.float32, T, 64, 64)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        res = expect_success(bs.greeks_batch_device(cd))
    assert bs.ordinal == ORD0 + 12
    fields = list(BlackScholes.BatchGreeks.model_fields)
    for name in fields:  # views of the one block the replay writes: poisoned, so an unwritten element shows
        getattr(res, name).fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(torch.stack([getattr(res, name) for name in fields], dim=1).cpu().numpy(), eager,
                      "replayed graph vs eager")
