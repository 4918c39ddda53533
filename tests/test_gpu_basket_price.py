"""Batched basket pricing (smc_basket_price / basket_price / BasketEngine.price): the [B][18] block of
basket_price_kernel against the CPU restatement.

The expectation takes the oracle's kernel-mode terminal rows (oracle.basket_kernel with N = 4: the kernel's own
streams, one per group of 4 paths, so the first P columns of a longer run are the P-path run's), restates the
table of include/spectralmc_hip.h in numpy float32 with the portable exp (oracle_exp2): F_i, df, K, the scales
s_i = F_i / f32(tot_i / P) from the kernel's own terminal sums, xs_i = x_i s_i, the basket in asset order, the
maximum and the minimum, the six payoffs; and sums them in float64 (numpy's pairwise order, not the kernel's:
hence the P 2^-52 bounds).  The exercise count is an integer: it is compared bit for bit, so one wrong
comparison or one scale off by an ulp shows.

The oracle is run on a path count rounded up to a multiple of 2048 (its terminal-sum loop walks whole
2048-path chunks of its terminal buffer) and truncated to P; its own terminal sums are used only where
P % 2048 == 0, where they are basket_kernel's (wg = 512) bit for bit."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.basket import PRICE_FIELDS, BasketConfig, BasketEngine, BasketPrices, basket_price, basket_targets
from tests.helpers import assert_rows_equal, poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7
ORD0 = 3
COLS = _lib.BASKET_PRICE_COLS
MEANS = (0, 1, 2, 3, 4, 5, 12, 13, 14)
NAMES = ("basket put", "basket call", "best-of put", "best-of call", "worst-of put", "worst-of call")
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _contracts(A: int, n: int) -> np.ndarray:
    """[n, 3A + 4] rows K, T, r, rho, X0.., d.., v.. (the first rows of any longer batch of the same A)."""
    rng = np.random.default_rng(2026 + A)
    rows = []
    for _ in range(n):
        x0 = rng.uniform(50, 150, A)
        k = x0.mean() * rng.uniform(0.8, 1.25)
        t, r, rho = rng.uniform(0.25, 2), rng.uniform(-0.02, 0.08), rng.uniform(-0.1, 0.8)
        d, v = rng.uniform(0, 0.04, A), rng.uniform(0.1, 0.6, A)
        rows.append([k, t, r, rho, *x0, *d, *v])
    out = np.array(rows, dtype=np.float64)
    out.setflags(write=False)
    return out


def _price(c: np.ndarray, A: int, T: int, P: int, math: int, norm: int, ordinal0: int = ORD0, seed: int = SEED,
           ordinal_dev: torch.Tensor | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(block [B, 18], terminal sums [B, A]) of one smc_basket_price call into NaN-poisoned outputs."""
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], COLS), torch.float64, DEV)
    tsum = poisoned((c.shape[0], A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price(_lib.ptr(cd), c.shape[0], A, T, P, seed, _lib.ptr(ordinal_dev), ordinal0, math,
                                           norm, _lib.ptr(out), _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tsum.cpu().numpy()


def _name(A: int, T: int, P: int, math: int, norm: int) -> str:
    return _lib.lib().smc_basket_price_kernel(A, T, P, math, norm).decode()


def _exp_any(x: np.ndarray) -> np.ndarray:
    """math::exp_any in portable math: exp2_any(x * f32(log2 e)) elementwise on a float32 array."""
    exp2 = _oracle.oracle.lib().oracle_exp2
    assert x.dtype == f32
    flat = [exp2(float(f32(v) * f32(1.44269502))) for v in x.ravel()]
    return np.array(flat, dtype=f32).reshape(x.shape)


def _stderr(s1: np.ndarray, s2: np.ndarray, P: int) -> np.ndarray:
    if P == 1:
        return np.zeros_like(s1)
    m = s1 / P
    return np.sqrt(np.maximum(s2 - P * m * m, 0.0) / (P - 1) / P)


def _restate(c: np.ndarray, A: int, x: np.ndarray, tsum: np.ndarray, norm: int) -> dict[str, np.ndarray]:
    """The 18 columns (and m^2 / var of the six payoffs, [B, 6]) from the raw terminal values x [B, A, P] f32 and
    the terminal sums [B, A] f64: every per-path value in float32, the sums in float64."""
    B, _, P = x.shape
    assert x.dtype == f32
    K, Tm, r = c[:, 0].astype(f32), c[:, 1].astype(f32), c[:, 2]
    X0, d = c[:, 4:4 + A], c[:, 4 + A:4 + 2 * A]
    df = _exp_any((-r).astype(f32) * Tm)
    wA = f32(1.0 / A)
    F = X0.astype(f32) * _exp_any((r[:, None] - d).astype(f32) * Tm[:, None])
    s = F / (tsum / float(P)).astype(f32) if norm else np.ones((B, A), dtype=f32)
    xs = x * s[:, :, None]
    bs, fs = np.zeros((B, P), dtype=f32), np.zeros(B, dtype=f32)
    for i in range(A):  # asset order
        bs = bs + xs[:, i, :]
        fs = fs + F[:, i]
    bk, mx, mn, Fb = bs * wA, xs.max(axis=1), xs.min(axis=1), fs * wA
    assert xs.dtype == f32 and bk.dtype == f32 and Fb.dtype == f32 and df.dtype == f32 and s.dtype == f32

    def pay(diff: np.ndarray) -> np.ndarray:
        v = (df[:, None] if diff.ndim == 2 else df) * np.maximum(diff, f32(0))
        assert v.dtype == f32
        return v.astype(np.float64)

    Kc = K[:, None]
    pays = [pay(Kc - bk), pay(bk - Kc), pay(Kc - mx), pay(mx - Kc), pay(Kc - mn), pay(mn - Kc)]
    s1 = np.stack([v.sum(axis=1) for v in pays], axis=1)
    s2 = np.stack([(v * v).sum(axis=1) for v in pays], axis=1)
    cols = np.empty((B, COLS))
    cols[:, :6] = s1 / P
    cols[:, 6:12] = _stderr(s1, s2, P)
    for col, v in ((12, bk), (13, mx), (14, mn)):
        cols[:, col] = v.astype(np.float64).sum(axis=1) / P
    cols[:, 15] = (bk < Kc).sum(axis=1) / P
    cols[:, 16], cols[:, 17] = pay(K - Fb), pay(Fb - K)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.square(s1 / P) / np.maximum(s2 / P - np.square(s1 / P), 1e-300)
    return {"cols": cols, "m2_over_var": rho}


@functools.lru_cache(maxsize=None)
def _terminal(A: int, T: int, P: int, B: int) -> tuple[np.ndarray, np.ndarray | None]:
    """The oracle's raw terminal values [B, A, P] f32 of _contracts(A, B) and, where P % 2048 == 0, its terminal
    sums in basket_kernel's order (else None)."""
    _oracle.build()
    c = _contracts(A, B)
    M = -(-P // 2048) * 512
    paths, tsum, _ = _oracle.basket_kernel(c, A, T, 4, M, SEED, ordinal0=ORD0, want_paths=True)
    x = np.ascontiguousarray(paths[:, :, -1, :P])
    x.setflags(write=False)
    return x, (tsum if P % 2048 == 0 else None)


@functools.lru_cache(maxsize=None)
def _got(A: int, T: int, P: int, norm: int, B: int, math: int = 0) -> tuple[np.ndarray, np.ndarray]:
    out = _price(_contracts(A, B), A, T, P, math, norm)
    for a in out:
        a.setflags(write=False)
    return out


# (A, T, P, norm, B)
CASES = [
    (4, 16, 4096, 1, 12),   # lds, two chunks
    (3, 5, 2048, 1, 12),    # odd A: a discarded normal
    (1, 3, 2048, 0, 12),    # A = 1, RAW
    (8, 2, 2048, 1, 12),    # A = 8
    (2, 4, 693, 1, 12),     # P % 4 != 0, a partial chunk
    (4, 1, 528, 0, 12),     # T = 1, RAW, a partial chunk
    (2, 3, 65536, 1, 3),    # parked block too large: replay by itself
    (4, 3, 2048, 1, 300),   # more contracts than CUs
]


def _expected_name(A: int, P: int, norm: int) -> str:
    if not norm:
        return "basket_price_kernel(raw)"
    return "basket_price_kernel(replay)" if (A, P) == (2, 65536) else "basket_price_kernel(lds)"


@pytest.mark.parametrize("A,T,P,norm,B", CASES)
def test_basket_price_matches_restatement(A, T, P, norm, B) -> None:
    got, tsum = _got(A, T, P, norm, B)
    assert _name(A, T, P, 0, norm) == _expected_name(A, P, norm)
    assert not np.isnan(got).any() and not np.isnan(tsum).any()
    x, oracle_tsum = _terminal(A, T, P, B)
    if oracle_tsum is not None:  # basket_kernel's terminal_sum order, bit for bit
        assert_rows_equal(tsum, oracle_tsum, "terminal sums")
    else:  # the f32 4-path partials against an f64 sum (test_basket_host's bound)
        np.testing.assert_allclose(tsum, x.astype(np.float64).sum(axis=2), rtol=1e-6, atol=0)
    want = _restate(_contracts(A, B), A, x, tsum, norm)
    w, rho = want["cols"], want["m2_over_var"]
    e = P * 2.0 ** -52
    zero_means = int((w[:, :6] == 0.0).sum())
    print(f"zero means {zero_means} of {6 * B}, largest m^2 / var {rho[w[:, :6] > 0].max():.2f}, exercise share "
          f"{w[:, 15].min():.3f} .. {w[:, 15].max():.3f}")
    with np.errstate(invalid="ignore", divide="ignore"):
        for col in MEANS:
            rel = np.abs(got[:, col] - w[:, col]) / np.abs(w[:, col])
            print(f"col {col}: max rel {np.nanmax(rel):.3e} (bound {e:.3e})")
        for col in range(6):
            tol = 8 * e * np.maximum(1.0, rho[:, col] / 2)
            err = np.abs(got[:, 6 + col] - w[:, 6 + col]) / w[:, 6 + col]
            print(f"col {6 + col}: max rel {np.nanmax(err):.3e}, max share of its bound {np.nanmax(err / tol):.3f}")
    # a kernel that returns zeros must not pass on 0 == 0: the basket columns are never zero, and at most a
    # quarter of the (contract, payoff) pairs (deep best-of puts and worst-of calls) are
    assert np.all(w[:, :2] > 0.0) and 4 * zero_means <= 6 * B
    # the exercise count is an integer over P paths: bit for bit
    assert_rows_equal(got[:, 15], w[:, 15], "exercise share")
    assert_rows_equal(got[:, 16:18], w[:, 16:18], "intrinsic values")
    # two f64 sums of P non-negative terms in different orders each err by at most (P - 1) 2^-53 relative
    for col in MEANS:
        np.testing.assert_allclose(got[:, col], w[:, col], rtol=e, atol=0, err_msg=f"col {col}")
    # the standard errors take D = sum v^2 - P m^2, which moves by e (1 + 3 rho) D with rho = m^2 / var, halved by
    # the square root (test_price_matches_restatement_f32): 8 e max(1, rho / 2)
    for col in range(6):
        tol = 8 * e * np.maximum(1.0, rho[:, col] / 2)
        assert np.all(np.abs(got[:, 6 + col] - w[:, 6 + col]) <= tol * w[:, 6 + col]), NAMES[col]


@pytest.mark.parametrize("A,T,P,norm,B", [c for c in CASES if c[3] and _expected_name(c[0], c[2], 1).endswith("(lds)")])
def test_basket_price_modes_agree_bitwise(A, T, P, norm, B) -> None:
    """Parked in LDS and replayed: the same values in the same order."""
    assert _name(A, T, P, 0, 1) == "basket_price_kernel(lds)"
    assert _name(A, T, P, _lib.PRICE_REPLAY, 1) == "basket_price_kernel(replay)"
    lds, lds_sum = _got(A, T, P, 1, B)
    replay, replay_sum = _price(_contracts(A, B), A, T, P, _lib.PRICE_REPLAY, 1)
    assert not np.isnan(replay).any()
    assert_rows_equal(replay, lds, "replay vs lds")
    assert_rows_equal(replay_sum, lds_sum, "terminal sums, replay vs lds")


@pytest.mark.parametrize("A,N,M", [(4, 64, 64), (3, 256, 8)])
def test_basket_price_ties_to_the_training_call(A, N, M) -> None:
    """The same seed and ordinals through smc_basket_train_targets (basket_kernel + basket_cf_kernel): its
    terminal sums bit for bit, and its k = 0 target, N times the mean put rounded once to f32."""
    T, B = 5, 12
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="portable")
    c = _contracts(A, B)
    got, tsum = _price(c, A, T, N * M, 0, 1)
    train_sum = poisoned((B, A), torch.float64, DEV)
    targets = basket_targets(torch.tensor(c, dtype=torch.float64, device=DEV), cfg, ordinal0=ORD0, terminal_sum=train_sum,
                             resident=False)
    torch.cuda.synchronize()
    assert_rows_equal(tsum, train_sum.cpu().numpy(), "terminal sums vs the training call")
    mean_put = targets[:, 0].real.double().cpu().numpy() / N
    rel = np.abs(mean_put - got[:, 0]) / got[:, 0]
    print(f"targets[:, 0] / N against column 0: max rel {rel.max():.3e} (bound {2.0 ** -22:.3e})")
    assert np.all(rel <= 2.0 ** -22)


def test_basket_price_is_deterministic_and_splits() -> None:
    A, T, P = 4, 16, 4096
    c = _contracts(A, 12)
    whole, whole_sum = _price(c, A, T, P, 0, 1, 100)
    assert not np.isnan(whole).any()
    again, again_sum = _price(c, A, T, P, 0, 1, 100)
    assert_rows_equal(again, whole, "run to run")
    assert_rows_equal(again_sum, whole_sum, "run to run, terminal sums")
    tail, tail_sum = _price(c[5:], A, T, P, 0, 1, 105)
    assert_rows_equal(tail, whole[5:], "batch split at contract 5")
    assert_rows_equal(tail_sum, whole_sum[5:], "batch split at contract 5, terminal sums")
    assert_rows_equal(_price(c[:5], A, T, P, 0, 1, 100)[0], whole[:5], "batch split at contract 5, head")
    for dev_part in (105, 40):  # the ordinal's offset on the device, all of it and part of it
        od = torch.tensor([dev_part], dtype=torch.int64, device=DEV)
        assert_rows_equal(_price(c[5:], A, T, P, 0, 1, 105 - dev_part, ordinal_dev=od)[0], whole[5:],
                          f"ordinal_dev = {dev_part}")
    other, other_sum = _price(c, A, T, P, 0, 1, 101)  # other ordinals are other streams
    assert not np.any(other_sum == whole_sum) and not np.array_equal(other[:, 0], whole[:, 0])


@pytest.mark.parametrize("A,T,P,norm,B", CASES)
def test_basket_price_orderings_and_parity(A, T, P, norm, B) -> None:
    c = _contracts(A, B)
    got, _ = _got(A, T, P, norm, B)
    assert np.all(got[:, 14] <= got[:, 12]) and np.all(got[:, 12] <= got[:, 13])  # worst <= basket <= best
    assert np.all(got[:, 3] >= got[:, 1]) and np.all(got[:, 1] >= got[:, 5])      # calls: best >= basket >= worst
    assert np.all(got[:, 4] >= got[:, 0]) and np.all(got[:, 0] >= got[:, 2])      # puts: worst >= basket >= best
    assert np.all(got[:, :12] >= 0.0)
    assert np.all(got[:, 15] >= 0.0) and np.all(got[:, 15] <= 1.0)
    if norm:
        K, Tm, r = c[:, 0], c[:, 1], c[:, 2]
        F = c[:, 4:4 + A] * np.exp((r[:, None] - c[:, 4 + A:4 + 2 * A]) * Tm[:, None])
        rel = np.abs(got[:, 12] / F.mean(axis=1) - 1)
        # every asset's mean sits on its forward; the per-path values carry three f32 roundings
        print(f"mean basket against the mean forward: max rel {rel.max():.3e} (bound {2.0 ** -21:.3e})")
        assert np.all(rel <= 2.0 ** -21)
        parity = got[:, 1] - got[:, 0] - np.exp(-r * Tm) * (got[:, 12] - K)
        bound = 2.0 ** -20 * np.maximum(K, got[:, 12])
        print(f"put-call parity: max share of its bound {np.max(np.abs(parity) / bound):.3f}")
        assert np.all(np.abs(parity) <= bound)


DEGENERATE_SHAPES = ((8, 256), (3, 2053))


@pytest.mark.parametrize("flag", [0, _lib.PRICE_REPLAY])
def test_basket_price_degenerate_rows(flag) -> None:
    """v = 0 (every path ends on its forwards, so each payoff is its intrinsic form: xs_i = x_i (F_i / mean x_i)
    carries three f32 roundings, within 2^-22 of the contract's scale max(K, max F_i)) and T = 0 (every value is
    X0_i exactly)."""
    A = 4
    x0 = [100.0, 80.0, 120.0, 90.0]
    c = np.array([[95.0, 2.0, 0.05, 0.3, *x0, 0.01, 0.0, 0.02, 0.03, 0, 0, 0, 0],
                  [120.0, 2.0, 0.05, 0.3, *x0, 0.01, 0.0, 0.02, 0.03, 0, 0, 0, 0],
                  [40.0, 0.0, 0.1, 0.5, 50.0, 30.0, 70.0, 50.0, 0, 0, 0, 0, 0.7, 0.2, 0.4, 0.1]])
    K, Tm, r = c[:, 0], c[:, 1], c[:, 2]
    F = c[:, 4:4 + A] * np.exp((r[:, None] - c[:, 4 + A:4 + 2 * A]) * Tm[:, None])
    df = np.exp(-r * Tm)
    under = np.stack([F.mean(axis=1), F.max(axis=1), F.min(axis=1)], axis=1)
    det = np.empty((3, 6))
    det[:, 0::2] = df[:, None] * np.maximum(K[:, None] - under, 0.0)
    det[:, 1::2] = df[:, None] * np.maximum(under - K[:, None], 0.0)
    scale = np.maximum(K, F.max(axis=1))
    for T, P in DEGENERATE_SHAPES:
        assert _name(A, T, P, flag, 1) == ("basket_price_kernel(replay)" if flag else "basket_price_kernel(lds)")
        got, tsum = _price(c, A, T, P, flag, 1, 0)
        assert not np.isnan(got).any()
        err = np.abs(got[:, :6] - det)
        print(f"T {T} P {P}: worst error / (2^-22 scale) {np.max(err / (2.0 ** -22 * scale[:, None])):.3f}")
        assert np.all(err <= 2.0 ** -22 * scale[:, None])
        assert np.all(got[:, 6:12] <= 1e-6 * K[:, None])
        # T = 0: exact
        assert_rows_equal(tsum[2], c[2, 4:4 + A] * P, "terminal sums at T = 0")
        assert got[2, 12] == 50.0 and got[2, 13] == 70.0 and got[2, 14] == 30.0
        assert got[2].tolist()[:6] == [0.0, 10.0, 0.0, 30.0, 10.0, 0.0]
        assert np.all(got[2, 6:12] == 0.0) and got[2, 15] == 0.0 and got[2, 16] == 0.0 and got[2, 17] == 10.0
        assert got[0, 15] == 0.0 and got[1, 15] == 1.0  # the forward basket lies above 95 and below 120


@pytest.mark.parametrize("flag", [0, _lib.PRICE_REPLAY])
def test_basket_price_identical_assets_at_full_correlation(flag) -> None:
    """A = 2, rho = 1, the same asset twice: the basket, the best and the worst are one value."""
    c = np.array([[100.0, 1.0, 0.03, 1.0, 100.0, 100.0, 0.01, 0.01, 0.3, 0.3],
                  [90.0, 0.5, 0.01, 1.0, 80.0, 80.0, 0.0, 0.0, 0.5, 0.5]])
    for T, P in DEGENERATE_SHAPES:
        got, tsum = _price(c, 2, T, P, flag, 1, 0)
        assert not np.isnan(got).any() and np.all(got[:, :2] > 0.0)
        assert_rows_equal(tsum[:, 0], tsum[:, 1], "terminal sums")
        for first in (0, 1, 6, 7):
            assert_rows_equal(got[:, first + 2], got[:, first], f"columns {first + 2} and {first}")
            assert_rows_equal(got[:, first + 4], got[:, first], f"columns {first + 4} and {first}")
        assert_rows_equal(got[:, 13], got[:, 12], "mean best and mean basket")
        assert_rows_equal(got[:, 14], got[:, 12], "mean worst and mean basket")


def test_basket_price_single_path_has_zero_stderr() -> None:
    for flag in (0, _lib.PRICE_REPLAY):
        got, _ = _price(_contracts(4, 12), 4, 4, 1, flag, 1, 0)
        assert not np.isnan(got).any()
        assert np.all(got[:, 6:12] == 0.0)
        assert np.all((got[:, 15] == 0.0) | (got[:, 15] == 1.0))


def test_basket_price_hw_math_close_to_portable() -> None:
    A, T, P, B = 4, 16, 4096, 32
    x, tsum = _terminal(A, T, P, B)
    want = _restate(_contracts(A, B), A, x, tsum, 1)["cols"]
    got, got_sum = _price(_contracts(A, B), A, T, P, _lib.MATH_HW, 1)
    assert not np.isnan(got).any() and not np.isnan(got_sum).any()
    for col in (0, 1, 3, 4, 12, 13, 14):  # batch norm-relative, the project's 1e-5 for hardware-transcendental f32 runs
        rel = float(np.linalg.norm(got[:, col] - want[:, col]) / np.linalg.norm(want[:, col]))
        print(f"col {col}: batch norm-relative {rel:.3e}")
        assert rel < 1e-5, col
    assert_rows_equal(got[:, 16:18], want[:, 16:18], "intrinsic values do not use the path math")


def test_basket_price_against_the_closed_form(oracle) -> None:
    """A = 1: the basket is the asset, and its put is Black's (test_price_against_the_closed_form's check)."""
    c = _contracts(1, 64)
    got, _ = _price(c, 1, 16, 65536, 0, 1)
    assert _name(1, 16, 65536, 0, 1) == "basket_price_kernel(replay)"
    assert not np.isnan(got).any()
    black = np.array([oracle.black_put(row[4], row[0], row[1], row[2], row[5], row[6]) for row in c.tolist()])
    z = np.abs(got[:, 0] - black) / got[:, 6]
    print(f"worst |put - black| / stderr {z.max():.2f}")
    assert np.all(np.abs(got[:, 0] - black) <= 5.0 * got[:, 6])
    # one asset: best and worst are the basket (the basket takes one more rounding, the product with f32(1))
    assert_rows_equal(got[:, [2, 3, 8, 9, 13]], got[:, [4, 5, 10, 11, 14]], "best-of and worst-of at A = 1")


def test_basket_price_python_api() -> None:
    A, T, N, M, B = 4, 16, 64, 64, 12
    c = _contracts(A, B)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="portable")
    res = basket_price(cd, cfg, ordinal0=ORD0)
    assert isinstance(res, BasketPrices)
    torch.cuda.synchronize()
    want, want_sum = _got(A, T, N * M, 1, B)
    assert res.block.shape == (B, COLS) and res.block.dtype == torch.float64 and res.block.is_cuda
    assert_rows_equal(res.block.cpu().numpy(), want, "basket_price vs the C call")
    assert_rows_equal(res.terminal_sum.cpu().numpy(), want_sum, "terminal sums")
    assert len(PRICE_FIELDS) == COLS
    for col, name in enumerate(PRICE_FIELDS):
        t = getattr(res, name)
        assert t.shape == (B,) and t.dtype == torch.float64 and t.is_cuda, name
        assert_rows_equal(t.cpu().numpy(), want[:, col], name)
    # replay: the same bits; n_paths: any positive count, not only the training call's
    assert_rows_equal(basket_price(cd, cfg, ordinal0=ORD0, replay=True).block.cpu().numpy(), want, "replay=True")
    odd = basket_price(cd, cfg, ordinal0=ORD0, n_paths=693)
    assert_rows_equal(odd.block.cpu().numpy(), _price(c, A, T, 693, 0, 1)[0], "n_paths = 693")
    # RAW through cfg.normalize
    raw_cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="portable",
                           normalize=False)
    assert_rows_equal(basket_price(cd, raw_cfg, ordinal0=ORD0).block.cpu().numpy(), _price(c, A, T, N * M, 0, 0)[0], "RAW")
    # math="hw" reaches the SMC_MATH_HW launch
    hw_cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="hw")
    hw = basket_price(cd, hw_cfg, ordinal0=ORD0).block.cpu().numpy()
    assert_rows_equal(hw, _price(c, A, T, N * M, _lib.MATH_HW, 1)[0], 'math="hw" vs SMC_MATH_HW')
    assert not np.array_equal(hw[:, 0], want[:, 0])
    # the empty batch: empty tensors, no launch
    empty = basket_price(cd[:0], cfg)
    assert empty.block.shape == (0, COLS) and empty.basket_put.shape == (0,) and empty.terminal_sum.shape == (0, A)
    # malformed tensors raise
    for bad in (cd[:, :5], cd.to(torch.float32), cd.reshape(-1), cd.cpu()):
        with pytest.raises(ValueError):
            basket_price(bad, cfg)
    with pytest.raises(ValueError):
        basket_price(cd, cfg, n_paths=0)


def test_basket_engine_price() -> None:
    cfg = BasketConfig(n_assets=3, timesteps=8, network_size=64, batches_per_mc_run=32, mc_seed=SEED, math="portable")
    eng = BasketEngine(cfg, 16, device=torch.device(DEV))
    eng.set_position(0, 0)
    eng.enqueue_step()
    got = eng.price()
    want = basket_price(eng.buffers.contracts, cfg)
    torch.cuda.synchronize()
    assert got.block.shape == (16, COLS) and not bool(torch.isnan(got.block).any())
    assert_rows_equal(got.block.cpu().numpy(), want.block.cpu().numpy(), "BasketEngine.price vs basket_price")
    # the training launch of the step made the same terminal sums (ordinals 0..15, P a multiple of 2048)
    assert_rows_equal(got.terminal_sum.cpu().numpy(), eng.terminal_sum.cpu().numpy(), "terminal sums of the step")
    other = eng.price(eng.buffers.contracts[:4], ordinal0=2, n_paths=100)
    assert_rows_equal(other.block.cpu().numpy(),
                      basket_price(eng.buffers.contracts[:4], cfg, ordinal0=2, n_paths=100).block.cpu().numpy(), "overrides")


def test_basket_price_call_is_capturable() -> None:
    A, T, P, B = 4, 16, 4096, 12
    eager, eager_sum = _got(A, T, P, 1, B)
    cd = torch.tensor(_contracts(A, B), dtype=torch.float64, device=DEV)
    out = poisoned((B, COLS), torch.float64, DEV)
    tsum = poisoned((B, A), torch.float64, DEV)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        _lib.check(_lib.lib().smc_basket_price(_lib.ptr(cd), B, A, T, P, SEED, None, ORD0, 0, 1, _lib.ptr(out),
                                               _lib.ptr(tsum), _lib.stream_handle()))
    assert bool(torch.isnan(out).all())  # capturing launches nothing
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(out.cpu().numpy(), eager, "replayed graph vs eager")
    assert_rows_equal(tsum.cpu().numpy(), eager_sum, "replayed graph vs eager, terminal sums")
