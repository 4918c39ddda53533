"""Path-dependent batched pricing (smc_gbm_price_paths / BlackScholes.price_paths_batch): the [B][20] block of
path_price_kernel against the CPU restatement.

The f32 expectation takes the oracle's kernel-mode path matrix and row sums (oracle.kernel_paths, wg = 512: the
kernel's own streams and row-sum order), restates the row scales s_t = F_t / f32(rowsum_t / P), the discount and
the strike in numpy float32 with the portable exp (oracle_exp2), walks the rows in float32 for the per-path sum,
maximum, minimum and knocked flag, takes the payoffs in float32 and sums them in float64 (numpy's pairwise
order, not the kernel's: hence the P 2^-52 bounds).  The knocked count is an integer: it is compared bit for
bit, so one wrong comparison or one row scale off by an ulp shows."""

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
from tests.helpers import ATOL_FLOAT64, RTOL_FLOAT64, assert_rows_equal, expect_success, poisoned
from tests.test_gpu_price import ORD0, SEED, _contracts, _engine, _inputs, _price, _stderr

pytestmark = pytest.mark.gpu

DEV = "cuda"
COLS = _lib.PATH_PRICE_COLS
MEANS = (0, 1, 2, 3, 4, 5, 6, 7, 16, 18, 19)
NAMES = ("asian put", "asian call", "knock-out put", "knock-out call", "lookback put", "lookback call", "put", "call")


_barriers = gr.barriers


def _paths(c: np.ndarray, T: int, P: int, scheme: int, norm: int, dtype: int = 0, ordinal0: int = 0,
           barriers: np.ndarray | None = None, seed: int = SEED, ordinal_dev: torch.Tensor | None = None) -> np.ndarray:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    bd = None if barriers is None else torch.tensor(barriers, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_price_paths(_lib.ptr(cd), _lib.ptr(bd), c.shape[0], T, P, seed, _lib.ptr(ordinal_dev),
                                              ordinal0, scheme, norm, dtype, _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _got(B: int, T: int, P: int, scheme: int, norm: int, dtype: int = 0, with_barriers: bool = True) -> np.ndarray:
    c = _contracts(B)
    out = _paths(c, T, P, scheme, norm, dtype, ORD0, _barriers(c) if with_barriers else None)
    out.setflags(write=False)
    return out


_time_grid = gr.time_grid
_block = gr.path_block


@functools.lru_cache(maxsize=None)
def _restated_f32(B: int, T: int, P: int, scheme: int, norm: int) -> dict[str, np.ndarray]:
    c = _contracts(B)
    return gr.path_price_f32(_oracle, c, _barriers(c), T, P, SEED, ORD0, scheme, norm)


def _restated_f64(B: int, T: int, P: int, scheme: int, norm: int) -> dict[str, np.ndarray]:
    _oracle.build()
    c = _contracts(B)
    paths, _, rs = _oracle.gbm_paths(c, T, P, SEED, ORD0, scheme, dtype="float64", want_paths=True)
    df = np.exp(-c[:, 3] * c[:, 2])
    if norm:
        F = c[:, 0][:, None] * np.exp((c[:, 3] - c[:, 4])[:, None] * _time_grid(c, T))
        paths = paths * (F / (rs / P))[:, :, None]
    bars = _barriers(c)
    return _block(paths, c[:, 1].copy(), df, bars[:, 0].copy(), bars[:, 1].copy())


# (B, T, P, scheme, norm)
F32_CASES = [
    (12, 16, 4096, 0, 1),    # two whole chunks, one sweep of 16 accumulator rows
    (12, 5, 693, 1, 1),      # simple Euler, odd T, ragged P % 4 != 0
    (12, 3, 2048, 0, 0),     # RAW: one pass
    (12, 1, 528, 0, 1),      # T = 1, a partial chunk
    (12, 40, 693, 0, 1),     # T beyond one block of accumulator rows (34 in f32): two sweeps
    (3, 4, 65536, 0, 1),     # 32 chunks per lane
    (300, 3, 2048, 0, 1),    # more contracts than CUs
]


@pytest.mark.parametrize("B,T,P,scheme,norm", F32_CASES)
def test_path_price_matches_restatement_f32(B, T, P, scheme, norm) -> None:
    want = _restated_f32(B, T, P, scheme, norm)
    got = _got(B, T, P, scheme, norm)
    name = _lib.lib().smc_gbm_price_paths_kernel(T, P, scheme, norm, 0).decode()
    assert name == ("path_price_kernel(replay)" if norm else "path_price_kernel(raw)")
    w, rho = want["cols"], want["m2_over_var"]
    assert not np.isnan(got).any()
    e = P * 2.0 ** -52
    print(f"knocked share {w[:, 17].min():.3f} .. {w[:, 17].max():.3f}, smallest payoff mean {w[:, :8].min():.3e}, "
          f"largest m^2 / var {rho.max():.2f}")
    with np.errstate(invalid="ignore"):  # 0 / 0 where a strike beyond the upper barrier leaves the knock-out call at 0
        for col in MEANS:
            rel = np.abs(got[:, col] - w[:, col]) / np.abs(w[:, col])
            print(f"col {col}: max rel {np.nanmax(rel):.3e} (bound {e:.3e})")
        for col in range(8):
            tol = 8 * e * np.maximum(1.0, rho[:, col] / 2)
            err = np.abs(got[:, 8 + col] - w[:, 8 + col]) / w[:, 8 + col]
            print(f"col {8 + col}: max rel {np.nanmax(err):.3e}, max share of its bound {np.nanmax(err / tol):.3f}")
    # the knocked count is an integer over P paths: bit for bit
    assert_rows_equal(got[:, 17], w[:, 17], "knocked share")
    # two f64 sums of P non-negative terms in different orders each err by at most (P - 1) 2^-53 relative
    for col in MEANS:
        np.testing.assert_allclose(got[:, col], w[:, col], rtol=e, atol=0, err_msg=f"col {col}")
    # the standard errors take D = sum v^2 - P m^2, which moves by e (1 + 3 rho) D with rho = m^2 / var, halved by
    # the square root (test_price_matches_restatement_f32): 8 e max(1, rho / 2)
    for col in range(8):
        tol = 8 * e * np.maximum(1.0, rho[:, col] / 2)
        assert np.all(np.abs(got[:, 8 + col] - w[:, 8 + col]) <= tol * w[:, 8 + col]), NAMES[col]


@pytest.mark.parametrize("B,T,P,scheme,norm", F32_CASES)
def test_path_price_ties_to_the_price_call(B, T, P, scheme, norm) -> None:
    got = _got(B, T, P, scheme, norm)
    price = _price(_contracts(B), T, P, scheme, norm, 0, ORD0)
    assert_rows_equal(got[:, [6, 7, 14, 15]], price[:, [0, 1, 3, 4]], "European columns vs smc_gbm_price")
    if T == 1:  # one monitoring date: the average, the maximum and the minimum are the terminal value
        assert_rows_equal(got[:, [0, 1, 8, 9]], got[:, [6, 7, 14, 15]], "Asian vs European at T = 1")
        assert_rows_equal(got[:, [4, 5, 12, 13]], got[:, [6, 7, 14, 15]], "lookback vs European at T = 1")
    free = _got(B, T, P, scheme, norm, 0, False)
    assert_rows_equal(free[:, [2, 3, 10, 11]], free[:, [6, 7, 14, 15]], "no barrier: knock-out vs European")
    assert np.all(free[:, 17] == 0.0)
    # the barriers touch the knock-out columns and the knocked share only
    rest = [0, 1, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16, 18, 19]
    assert_rows_equal(free[:, rest], got[:, rest], "columns that do not depend on the barriers")


@pytest.mark.parametrize("B,T,P,scheme,norm", F32_CASES)
def test_path_price_meaning(B, T, P, scheme, norm) -> None:
    c = _contracts(B)
    got = _got(B, T, P, scheme, norm)
    if norm:  # every row's mean sits on its forward, so the mean average is the mean forward
        F = c[:, 0][:, None] * np.exp((c[:, 3] - c[:, 4])[:, None] * _time_grid(c, T))
        assert np.max(np.abs(got[:, 16] / F.mean(axis=1) - 1)) < 1e-6
    for side in (0, 1):  # lookback >= European >= knock-out >= 0
        assert np.all(got[:, 4 + side] >= got[:, 6 + side]), side
        assert np.all(got[:, 6 + side] >= got[:, 2 + side]), side
        assert np.all(got[:, 2 + side] >= 0.0), side
    assert np.all(got[:, 19] <= got[:, 16]) and np.all(got[:, 16] <= got[:, 18])
    assert np.all(got[:, 17] > 0.0) and np.all(got[:, 17] < 1.0)


def test_path_price_is_deterministic_and_splits() -> None:
    c = _contracts(12)
    bars = _barriers(c)
    T, P = 16, 4096
    whole = _paths(c, T, P, 0, 1, 0, 100, bars)
    assert not np.isnan(whole).any()
    assert_rows_equal(_paths(c, T, P, 0, 1, 0, 100, bars), whole, "run to run")
    assert_rows_equal(_paths(c[5:], T, P, 0, 1, 0, 105, bars[5:]), whole[5:], "batch split at contract 5")
    assert_rows_equal(_paths(c[:5], T, P, 0, 1, 0, 100, bars[:5]), whole[:5], "batch split at contract 5, head")
    for dev_part in (105, 40):  # the ordinal's offset on the device, all of it and part of it
        od = torch.tensor([dev_part], dtype=torch.int64, device=DEV)
        assert_rows_equal(_paths(c[5:], T, P, 0, 1, 0, 105 - dev_part, bars[5:], ordinal_dev=od), whole[5:],
                          f"ordinal_dev = {dev_part}")
    other = _paths(c, T, P, 0, 1, 0, 101, bars)  # other ordinals are other streams
    assert not np.array_equal(other[:, 16], whole[:, 16]) and not np.array_equal(other[:, 0], whole[:, 0])


@pytest.mark.parametrize("B,T,P,scheme,norm", [(6, 16, 4096, 0, 1), (6, 7, 1024, 1, 0), (2, 40, 693, 0, 1)])
def test_path_price_matches_oracle_f64(B, T, P, scheme, norm) -> None:
    want = _restated_f64(B, T, P, scheme, norm)
    got = _got(B, T, P, scheme, norm, 1)
    w, rho = want["cols"], want["m2_over_var"]
    assert not np.isnan(got).any()
    # a path would have to lie within ~1e-10 relative of a barrier to change sides
    assert_rows_equal(got[:, 17], w[:, 17], "knocked share")
    for col in MEANS:  # the project's f64 tolerance
        np.testing.assert_allclose(got[:, col], w[:, col], rtol=1e-10, atol=0, err_msg=f"col {col}")
    for col in range(8):
        tol = 1e-10 * (1 + 2 * rho[:, col])
        assert np.all(np.abs(got[:, 8 + col] - w[:, 8 + col]) <= tol * np.abs(w[:, 8 + col])), NAMES[col]


def test_path_price_hw_math_close_to_portable() -> None:
    """Hardware transcendentals against the portable restatement.  The knock-out columns and the knocked share
    are discontinuous in the path values (a path within rounding of a barrier may change sides), so this check
    of them is deliberately loose, three of their own standard errors: the barrier logic itself is pinned bit
    for bit by test_path_price_matches_restatement_f32."""
    B, T, P = 32, 16, 4096
    want = _restated_f32(B, T, P, 0, 1)["cols"]
    c = _contracts(B)
    got = _paths(c, T, P, _lib.MATH_HW, 1, 0, ORD0, _barriers(c))
    assert not np.isnan(got).any()
    for col in (0, 1, 4, 5, 6, 7, 16, 18, 19):  # batch norm-relative, the project's 1e-5 for hardware f32 runs
        rel = float(np.linalg.norm(got[:, col] - want[:, col]) / np.linalg.norm(want[:, col]))
        print(f"col {col}: batch norm-relative {rel:.3e}")
        assert rel < 1e-5, col
    for col in (2, 3):  # (a strike beyond the upper barrier: the knock-out call and its standard error are both 0)
        diff, se = np.abs(got[:, col] - want[:, col]), want[:, 8 + col]
        print(f"col {col}: worst |hw - portable| / stderr {np.max(diff[se > 0] / se[se > 0]):.3e}")
        assert np.all(diff <= 3.0 * se), col
    q = want[:, 17]
    assert np.all(np.abs(got[:, 17] - q) <= 3 * np.sqrt(q * (1 - q) / P))


@pytest.mark.parametrize("dtype", [0, 1])
def test_path_price_degenerate_contracts(dtype) -> None:
    """v = 0 and T = 0 (test_price_degenerate_contracts' rows): every path sits on its forward at every date.  The
    deterministic values are the payoffs of the row forwards F_t taken in the sim dtype (sum over t in that
    dtype, / T, max, min; f32 with the portable exp).  The kernel's xs_t = x (F_t / mean x) with mean x = x exactly
    is F_t after two roundings, which the sum over t averages: within 2^-22 of the contract's scale max(K, F)."""
    c = np.array([[100.0, 95.0, 2.0, 0.05, 0.01, 0.0], [50.0, 40.0, 0.0, 0.1, 0.0, 0.7],
                  [100.0, 120.0, 2.0, 0.05, 0.01, 0.0]])
    real = np.float32 if dtype == 0 else np.float64
    _oracle.build()
    exp2 = _oracle.oracle.lib().oracle_exp2

    def exp_any(x: np.ndarray) -> np.ndarray:
        if dtype == 1:
            return np.exp(x)
        flat = [exp2(float(np.float32(v) * np.float32(1.44269502))) for v in x.ravel()]
        return np.array(flat, dtype=np.float32).reshape(x.shape)

    Fend = c[:, 0] * np.exp((c[:, 3] - c[:, 4]) * c[:, 2])
    scale = np.maximum(c[:, 1], Fend)
    hi, lo = np.maximum(c[:, 0], Fend), np.minimum(c[:, 0], Fend)
    far = np.stack([0.5 * lo, 2.0 * hi], axis=1)      # the forward curve lies strictly inside: nothing knocked
    above = np.stack([1.5 * hi, 4.0 * hi], axis=1)    # the lower barrier lies above it: everything knocked
    for T, P in ((8, 256), (3, 2053)):
        F = c[:, 0].astype(real)[:, None] * exp_any((c[:, 3] - c[:, 4]).astype(real)[:, None] * _time_grid(c, T).astype(real))
        df = exp_any((-c[:, 3]).astype(real) * c[:, 2].astype(real))
        K = c[:, 1].astype(real)
        assert F.dtype == real and df.dtype == real
        a = np.zeros(3, dtype=real)
        for t in range(T):
            a = a + F[:, t]
        avg, mx, mn, last = a / real(T), F.max(axis=1), F.min(axis=1), F[:, -1]
        zero = real(0)
        det = np.stack([df * np.maximum(K - avg, zero), df * np.maximum(avg - K, zero), df * np.maximum(K - mn, zero),
                        df * np.maximum(mx - K, zero), df * np.maximum(K - last, zero), df * np.maximum(last - K, zero)],
                       axis=1).astype(np.float64)
        for bars, share in ((far, 0.0), (above, 1.0), (None, 0.0)):
            got = _paths(c, T, P, 0, 1, dtype, 0, bars)
            assert not np.isnan(got).any()
            err = np.abs(got[:, [0, 1, 4, 5, 6, 7]] - det)
            print(f"T {T} P {P}: worst error / (2^-22 scale) {np.max(err / (2.0 ** -22 * scale[:, None])):.3f}")
            assert np.all(err <= 2.0 ** -22 * scale[:, None])
            assert np.all(got[:, 8:16] <= 1e-6 * c[:, 1:2])
            assert np.all(got[:, 17] == share)
            if share == 0.0:
                assert_rows_equal(got[:, [2, 3, 10, 11]], got[:, [6, 7, 14, 15]], "nothing knocked")
            else:
                assert np.all(got[:, [2, 3, 10, 11]] == 0.0)
            # T = 0: every value is X0 exactly
            assert got[1, 16] == 50.0 and got[1, 18] == 50.0 and got[1, 19] == 50.0 and got[1, 0] == 0.0
            assert got[1, 1] == 10.0 and got[1, 5] == 10.0 and got[1, 7] == 10.0


def test_path_price_single_path_has_zero_stderr() -> None:
    c = _contracts(12)
    got = _paths(c, 4, 1, 0, 1, 0, 0, _barriers(c))
    assert not np.isnan(got).any()
    assert np.all(got[:, 8:16] == 0.0)
    assert np.all((got[:, 17] == 0.0) | (got[:, 17] == 1.0))


def _torch_reference(eng: BlackScholes, inp: BlackScholes.Inputs, lower: float, upper: float) -> dict[str, float]:
    """The parent route for one contract: the stored [T, P] matrix, reduced with torch."""
    sims = expect_success(eng._simulate(inp)).sims.to(torch.float64)
    T, P = sims.shape
    avg, mx, mn, last = sims.sum(dim=0) / T, sims.max(dim=0).values, sims.min(dim=0).values, sims[-1]
    ko = ((sims <= lower) | (sims >= upper)).any(dim=0)
    df = float(np.exp(-inp.r * inp.T))
    zero = torch.zeros((), dtype=torch.float64, device=sims.device)
    put, call = df * torch.maximum(inp.K - last, zero), df * torch.maximum(last - inp.K, zero)
    pays = {"asian_put": df * torch.maximum(inp.K - avg, zero), "asian_call": df * torch.maximum(avg - inp.K, zero),
            "knock_out_put": torch.where(ko, zero, put), "knock_out_call": torch.where(ko, zero, call),
            "lookback_put": df * torch.maximum(inp.K - mn, zero), "lookback_call": df * torch.maximum(mx - inp.K, zero),
            "put_price": put, "call_price": call}
    out = {}
    for name, v in pays.items():
        out[name] = float(v.mean())
        out[name + "_stderr"] = float(v.std(unbiased=True) / np.sqrt(P))
    out.update(mean_average=float(avg.mean()), knocked_share=float(ko.double().mean()), mean_max=float(mx.mean()),
               mean_min=float(mn.mean()))
    return out


def test_price_paths_batch_python_api() -> None:
    batch, loop = _engine(Precision.float64, 8, 64, 64, skip=3), _engine(Precision.float64, 8, 64, 64, skip=3)
    c = _contracts(12)
    cs = _inputs(c)
    bars = [tuple(row) for row in _barriers(c).tolist()]
    assert expect_success(batch.price_paths_batch([])) == [] and batch.ordinal == 3
    assert expect_success(batch.price_paths_batch([], [])) == [] and batch.ordinal == 3
    got = expect_success(batch.price_paths_batch(cs, bars))
    want = [_torch_reference(loop, inp, lo, up) for inp, (lo, up) in zip(cs, bars)]
    assert len(got) == len(cs) and all(isinstance(g, BlackScholes.HostPathPrices) for g in got)
    fields = list(BlackScholes.PathBatchPrices.model_fields)
    assert len(fields) == COLS and set(want[0]) == set(fields)
    for name in fields:
        if name == "knocked_share":
            assert [g.knocked_share for g in got] == [w[name] for w in want]
            assert 0.0 < min(g.knocked_share for g in got) and max(g.knocked_share for g in got) < 1.0
        else:
            np.testing.assert_allclose([getattr(g, name) for g in got], [w[name] for w in want], rtol=RTOL_FLOAT64,
                                       atol=ATOL_FLOAT64, err_msg=name)
    for g in got:
        assert g.knock_in_put == g.put_price - g.knock_out_put
        assert g.knock_in_call == g.call_price - g.knock_out_call
    # both consumed len(cs) normal streams, and go on alike
    for eng in (batch, loop):
        assert expect_success(eng.snapshot()).sim_params.skip == 3 + len(cs)
    assert expect_success(batch.price_to_host(cs[0])) == expect_success(loop.price_to_host(cs[0]))
    # without barriers nothing is knocked
    free = expect_success(_engine(Precision.float64, 8, 64, 64, skip=3).price_paths_batch(cs))
    for f, g in zip(free, got):
        assert f.knocked_share == 0.0 and f.knock_in_put == 0.0 and f.knock_out_call == f.call_price
        assert f.asian_put == g.asian_put and f.lookback_call == g.lookback_call and f.put_price == g.put_price
    # the device form: [B] f64 tensors on the device, the same launch
    fresh = _engine(Precision.float64, 8, 64, 64, skip=3)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    bd = torch.tensor(_barriers(c), dtype=torch.float64, device=DEV)
    dev = expect_success(fresh.price_paths_batch_device(cd, bd))
    assert fresh.ordinal == 3 + len(cs)
    for name in fields:
        t = getattr(dev, name)
        assert t.shape == (len(cs),) and t.dtype == torch.float64 and t.is_cuda, name
        assert t.cpu().tolist() == [getattr(g, name) for g in got], name
    empty = expect_success(fresh.price_paths_batch_device(cd[:0], bd[:0]))
    assert empty.asian_put.shape == (0,) and fresh.ordinal == 3 + len(cs)
    # malformed tensors raise before any ordinal is consumed
    for bad in (bd[:, :1], torch.cat([bd, bd], dim=1), bd.to(torch.float32), bd.cpu(), bd[:5], bd.reshape(-1)):
        with pytest.raises(ValueError):
            fresh.price_paths_batch_device(cd, bad)
    for bad in (cd[:, :5], cd.to(torch.float32), cd.cpu()):
        with pytest.raises(ValueError):
            fresh.price_paths_batch_device(bad, None)
    with pytest.raises(ValueError):
        fresh.price_paths_batch(cs, bars[:5])
    assert fresh.ordinal == 3 + len(cs)
    # hardware math is a float32 mode: the f64 engine reports the C ABI's status
    fresh.price_batch_math = "hw"
    with pytest.raises(_lib.SmcError) as exc:
        fresh.price_paths_batch_device(cd, bd)
    assert exc.value.code == _lib.SMC_ERR_INVALID_ARGUMENT and fresh.ordinal == 3 + len(cs)


def test_price_paths_batch_reports_an_invalid_normal_buffer() -> None:
    from spectralmc_amd.errors.gbm import NormalsUnavailable
    from spectralmc_amd.result import Failure
    from tests.helpers import make_black_scholes_config, make_simulation_params

    sp = make_simulation_params(timesteps=2, network_size=4, batches_per_mc_run=2, buffer_size=1000)
    bs = BlackScholes(make_black_scholes_config(sim_params=sp))
    cs = _inputs(_contracts(12))[:2]
    one = bs.price_to_host(cs[0])
    cd = torch.tensor(_contracts(12)[:2], dtype=torch.float64, device=DEV)
    bd = torch.tensor(_barriers(_contracts(12)[:2]), dtype=torch.float64, device=DEV)
    for res in (bs.price_paths_batch(cs), bs.price_paths_batch([]), bs.price_paths_batch(cs, [(1.0, 2.0)] * 2),
                bs.price_paths_batch_device(cd), bs.price_paths_batch_device(cd, bd)):
        assert isinstance(res, Failure) and isinstance(res.error, NormalsUnavailable)
        assert res.error == one.error
    assert bs.ordinal == 0


def test_path_price_call_is_capturable() -> None:
    c = _contracts(12)
    T, P = 16, 4096
    eager = _got(12, T, P, 0, 1)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    bd = torch.tensor(_barriers(c), dtype=torch.float64, device=DEV)
    out = poisoned((12, COLS), torch.float64, DEV)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        _lib.check(_lib.lib().smc_gbm_price_paths(_lib.ptr(cd), _lib.ptr(bd), 12, T, P, SEED, None, ORD0, 0, 1, 0,
                                                  _lib.ptr(out), _lib.stream_handle()))
    assert bool(torch.isnan(out).all())  # capturing launches nothing
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(out.cpu().numpy(), eager, "replayed graph vs eager")
