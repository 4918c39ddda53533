"""Batched basket Greeks (smc_basket_greeks / basket_greeks / BasketEngine.greeks): the [B][8A + 16] block and the
[B][3][A] pass-1 sums of basket_greeks_kernel.

Bit for bit where the kernel promises it (the terminal sums against the oracle, the price columns against
smc_basket_price, lds against replay, run to run, under a split of the batch, the ordinal on the host or on the device,
a replayed graph), within stated rounding bounds against the CPU restatement of the header's table
(tests/helpers/basket_greeks_restate.py: numpy float32 on the oracle's kernel-mode terminal values, portable exp and
log, float64 sums in numpy's pairwise order: hence the P 2^-52 bounds), and within a measured share of each column's
standard error against the independent float64 reference (tests/helpers/basket_greeks_reference.py)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.basket import BasketConfig, BasketEngine, BasketGreeks, basket_greeks, basket_greeks_fields
from tests.helpers import assert_rows_equal, poisoned
from tests.helpers import basket_greeks_cases as cases
from tests.helpers import basket_greeks_reference as gr
from tests.helpers import basket_greeks_restate as rs
from tests.helpers import basket_reference as br
from tests.helpers import instantiations as inst

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, ORD0, CASES = cases.SEED, cases.ORD0, cases.CASES
REPLAY = _lib.PRICE_REPLAY
f32 = np.float32


def _greeks(c: np.ndarray, A: int, T: int, P: int, math: int, norm: int, ordinal0: int = ORD0, seed: int = SEED,
            ordinal_dev: torch.Tensor | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(block [B, 8A + 16], sums [B, 3, A]) of one smc_basket_greeks call into NaN-poisoned outputs."""
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], 8 * A + 16), torch.float64, DEV)
    sums = poisoned((c.shape[0], 3, A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_greeks(_lib.ptr(cd), c.shape[0], A, T, P, seed, _lib.ptr(ordinal_dev), ordinal0, math,
                                            norm, _lib.ptr(out), _lib.ptr(sums), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), sums.cpu().numpy()


def _price(c: np.ndarray, A: int, T: int, P: int, math: int, norm: int, ordinal0: int = ORD0) -> tuple[np.ndarray, np.ndarray]:
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    out = poisoned((c.shape[0], _lib.BASKET_PRICE_COLS), torch.float64, DEV)
    tsum = poisoned((c.shape[0], A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price(_lib.ptr(cd), c.shape[0], A, T, P, SEED, None, ordinal0, math, norm,
                                           _lib.ptr(out), _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tsum.cpu().numpy()


def _name(A: int, T: int, P: int, math: int, norm: int) -> str:
    return _lib.lib().smc_basket_greeks_kernel(A, T, P, math, norm).decode()


def _expected_name(A: int, P: int, norm: int) -> str:
    if not norm:
        return "basket_greeks_kernel(raw)"
    return "basket_greeks_kernel(replay)" if (A, P) == (2, 65536) else "basket_greeks_kernel(lds)"


@functools.lru_cache(maxsize=None)
def _terminal(A: int, T: int, P: int, B: int) -> tuple[np.ndarray, np.ndarray | None]:
    """The oracle's raw terminal values [B, A, P] f32 of cases.contracts(A, B) and, where P % 2048 == 0, its terminal
    sums in basket_kernel's order (else None): tests/test_gpu_basket_price.py's _terminal."""
    _oracle.build()
    paths, tsum, _ = _oracle.basket_kernel(cases.contracts(A, B), A, T, 4, -(-P // 2048) * 512, SEED, ordinal0=ORD0,
                                           want_paths=True)
    x = np.ascontiguousarray(paths[:, :, -1, :P])
    x.setflags(write=False)
    return x, (tsum if P % 2048 == 0 else None)


@functools.lru_cache(maxsize=None)
def _got(A: int, T: int, P: int, norm: int, B: int, math: int = 0) -> tuple[np.ndarray, np.ndarray]:
    out = _greeks(cases.contracts(A, B), A, T, P, math, norm)
    for a in out:
        a.setflags(write=False)
    return out


def _stderr_cols(A: int) -> list[int]:
    n = 4 * A + 6
    return list(range(n, 2 * n)) + [2 * n + 2, 2 * n + 3]


# --------------------------------------------------------------------------- 1. the restatement, portable math
@pytest.mark.parametrize("A,T,P,norm,B", CASES)
def test_basket_greeks_match_restatement(A, T, P, norm, B) -> None:
    c = cases.contracts(A, B)
    got, sums = _got(A, T, P, norm, B)
    assert _name(A, T, P, 0, norm) == _expected_name(A, P, norm)
    assert got.shape == (B, 8 * A + 16) and not np.isnan(got).any() and not np.isnan(sums).any()
    x, oracle_tsum = _terminal(A, T, P, B)
    if oracle_tsum is not None:  # basket_kernel's terminal_sum order, bit for bit
        assert_rows_equal(sums[:, 0], oracle_tsum, "terminal sums")
    else:  # the f32 4-path partials against an f64 sum (test_gpu_basket_price's bound)
        np.testing.assert_allclose(sums[:, 0], x.astype(np.float64).sum(axis=2), rtol=1e-6, atol=0)
    # the constants come from the kernel's own pass-1 sums: f32(av), f32(aT) and f32(ac) are roundings of functions
    # of them, and a one-ulp move of any (which a sum-order difference can cause) would move every path's term
    r = rs.restate(_oracle, c, A, x, norm, sums)
    e = P * 2.0 ** -52
    if norm:
        for q, name in ((1, "xl"), (2, "xc")):
            want, bound = r[name].sum(axis=2), e * np.abs(r[name]).sum(axis=2)
            err = np.abs(sums[:, q] - want)
            with np.errstate(divide="ignore", invalid="ignore"):
                print(f"s{name}: max share of its bound {np.max(np.where(err == 0, 0.0, err / bound)):.3e}")
            assert np.all(err <= bound), name
            # asset 0 is the first driver whatever rho is (row 0 of G is 0), so c_0 = 0
            assert np.all(want[:, 1 if q == 2 else 0:] != 0.0) and (q == 1 or np.all(want[:, 0] == 0.0))
    else:
        assert np.all(sums[:, 1:] == 0.0)
    w = r["cols"]
    names = basket_greeks_fields(A)
    for term in range(4 * A + 8):
        col, se_col = rs.term_columns(A, term)
        err, bound = np.abs(got[:, col] - w[:, col]), r["bound"][term]
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(err == 0, 0.0, err / bound)
        print(f"{names[col]}: max share of its bound {share.max():.3e}")
        assert np.all(err <= bound), (names[col], int(np.argmax(share)))
        used = rs.check_stderr(got[:, se_col], w[:, se_col], r, term, P, names[col])
        print(f"{names[se_col]}: max share of its bound {used:.3f}")
    # a kernel that returns zeros must not pass on 0 == 0: every contract has paths on both sides of the strike, so
    # no delta or vega column is zero (at A = 1 under NORMALIZE the two vegas are equal and far from zero)
    assert np.all(got[:, :4 * A] != 0.0) and np.all(w[:, :4 * A] != 0.0)
    assert np.all(got[:, 4 * A:4 * A + 4] != 0.0)
    n = 4 * A + 6
    if A == 1:
        assert np.all(got[:, [n - 2, n - 1, 2 * n - 2, 2 * n - 1]] == 0.0)
    else:
        assert np.all(got[:, n - 2:n] != 0.0)


# --------------------------------------------------------------------------- 2. ties to the price call
@pytest.mark.parametrize("flag", [0, REPLAY])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("A,T,P", [(4, 16, 4096), (2, 4, 693), (8, 2, 2048)])
def test_basket_greeks_price_columns_are_the_price_call(A, T, P, norm, flag) -> None:
    c = cases.contracts(A, 12)
    got, sums = _greeks(c, A, T, P, flag, norm)
    price, tsum = _price(c, A, T, P, flag, norm)
    assert not np.isnan(got).any() and not np.isnan(price).any()
    n = 4 * A + 6
    assert_rows_equal(got[:, 2 * n:], price[:, [0, 1, 6, 7]], "columns 2n .. 2n + 3 vs smc_basket_price 0, 1, 6, 7")
    assert_rows_equal(sums[:, 0], tsum, "terminal sums vs smc_basket_price")


# --------------------------------------------------------------------------- 3. modes
@pytest.mark.parametrize("A,T,P,norm,B", [c for c in CASES if c[3] and _expected_name(c[0], c[2], 1).endswith("(lds)")])
def test_basket_greeks_modes_agree_bitwise(A, T, P, norm, B) -> None:
    """Parked in LDS and replayed: the same values in the same order, in one payoff pass or in several."""
    assert _name(A, T, P, 0, 1) == "basket_greeks_kernel(lds)"
    assert _name(A, T, P, REPLAY, 1) == "basket_greeks_kernel(replay)"
    lds, lds_sums = _got(A, T, P, 1, B)
    replay, replay_sums = _greeks(cases.contracts(A, B), A, T, P, REPLAY, 1)
    assert not np.isnan(replay).any()
    assert_rows_equal(replay, lds, "replay vs lds")
    assert_rows_equal(replay_sums, lds_sums, "pass-1 sums, replay vs lds")


# --------------------------------------------------------------------------- 4. determinism and splitting
@pytest.mark.parametrize("A,T,P", [(4, 16, 4096), (5, 3, 2053)])
def test_basket_greeks_are_deterministic_and_split(A, T, P) -> None:
    c = cases.contracts(A, 12)
    whole, whole_sums = _greeks(c, A, T, P, 0, 1, 100)
    assert not np.isnan(whole).any()
    again, again_sums = _greeks(c, A, T, P, 0, 1, 100)
    assert_rows_equal(again, whole, "run to run")
    assert_rows_equal(again_sums, whole_sums, "run to run, sums")
    tail, tail_sums = _greeks(c[5:], A, T, P, 0, 1, 105)
    assert_rows_equal(tail, whole[5:], "batch split at contract 5")
    assert_rows_equal(tail_sums, whole_sums[5:], "batch split at contract 5, sums")
    assert_rows_equal(_greeks(c[:5], A, T, P, 0, 1, 100)[0], whole[:5], "batch split at contract 5, head")
    for dev_part in (105, 40):  # the ordinal's offset on the device, all of it and part of it
        od = torch.tensor([dev_part], dtype=torch.int64, device=DEV)
        assert_rows_equal(_greeks(c[5:], A, T, P, 0, 1, 105 - dev_part, ordinal_dev=od)[0], whole[5:],
                          f"ordinal_dev = {dev_part}")
    other, other_sums = _greeks(c, A, T, P, 0, 1, 101)  # other ordinals are other streams
    moving = np.ones((3, A), dtype=bool)
    moving[2, 0] = False  # sxc_0 is 0 whatever the stream: asset 0 is the first driver at every rho
    assert not np.any(other_sums[:, moving] == whole_sums[:, moving]) and np.all(whole_sums[:, 2, 0] == 0.0)
    assert not np.array_equal(other[:, 0], whole[:, 0])


# --------------------------------------------------------------------------- 5. degenerate rows
DEGENERATE_SHAPES = ((8, 256), (3, 2053))


@pytest.mark.parametrize("flag", [0, REPLAY])
@pytest.mark.parametrize("norm", [0, 1])
def test_basket_greeks_degenerate_rows(norm, flag) -> None:
    """One asset without volatility (its vega and its error exactly 0, the four correlation columns NaN, everything
    else finite and the other vegas live), and T = 0 (every value is X0_i exactly: the call is in the money)."""
    A = 4
    x0 = [100.0, 80.0, 120.0, 90.0]
    c = np.array([[95.0, 2.0, 0.05, 0.3, *x0, 0.01, 0.0, 0.02, 0.03, 0.2, 0.3, 0.0, 0.25],
                  [40.0, 0.0, 0.1, 0.5, 50.0, 30.0, 70.0, 50.0, 0, 0, 0, 0, 0.7, 0.2, 0.4, 0.1]])
    n = 4 * A + 6
    corr = [n - 2, n - 1, 2 * n - 2, 2 * n - 1]
    rest = [k for k in range(2 * n + 4) if k not in corr]
    for T, P in DEGENERATE_SHAPES:
        got, sums = _greeks(c, A, T, P, flag, norm, 0)
        v0 = got[0]
        assert np.isnan(v0[corr]).all() and np.isfinite(v0[rest]).all() and np.isfinite(sums).all()
        assert np.all(v0[[2 * A + 2, 3 * A + 2, n + 2 * A + 2, n + 3 * A + 2]] == 0.0)  # asset 2: vega and its error
        live = [2 * A + i for i in (0, 1, 3)] + [3 * A + i for i in (0, 1, 3)]
        assert np.all(v0[live] != 0.0) and np.all(v0[[n + k for k in live]] > 0.0)
        assert np.all(sums[0, 2] == 0.0)  # no driver is recovered: g = g0 = 0
        t0 = got[1]
        assert np.isfinite(t0).all()
        assert t0[2 * n] == 0.0 and t0[2 * n + 1] == 10.0 and np.all(t0[_stderr_cols(A)] <= 1e-6)
        assert_rows_equal(sums[1, 0], np.array([50.0, 30.0, 70.0, 50.0]) * P, "terminal sums at T = 0")
        put_cols = list(range(0, A)) + list(range(2 * A, 3 * A)) + [4 * A, 4 * A + 2, 4 * A + 4]
        assert np.all(t0[put_cols] == 0.0)                       # nothing exercised on the put side
        np.testing.assert_allclose(t0[A:2 * A], 0.25, rtol=2.0 ** -22)  # d call / d X0_i = df xs_i / (A X0_i) = 1 / 4
        assert np.all(t0[3 * A:4 * A] == 0.0) and t0[4 * A + 1] == 0.0  # L = 0 and T K df = 0: no vega, no rho
        # theta: rr call - sT, with hT_i = aT_i alone (mu_i / 2 under RAW, r - d_i under NORMALIZE)
        v = c[1, 4 + 2 * A:]
        aT = np.full(A, 0.1) if norm else (0.1 - 0.5 * v * v) / 2.0
        want_theta = 0.1 * 10.0 - np.sum(c[1, 4:4 + A] * aT) / A
        assert abs(t0[4 * A + 3] - want_theta) <= 64 * 2.0 ** -22 * 50.0, (t0[4 * A + 3], want_theta)


@pytest.mark.parametrize("flag", [0, REPLAY])
def test_basket_greeks_single_asset_has_no_correlation(flag) -> None:
    c = cases.contracts(1, 12).copy()
    c[3, 6] = 0.0  # and not NaN where its one asset is deterministic either
    for norm in (0, 1):
        got, sums = _greeks(c, 1, 3, 2048, flag, norm)
        assert not np.isnan(got).any() and not np.isnan(sums).any()
        assert np.all(got[:, [8, 9, 18, 19]] == 0.0) and np.all(sums[:, 2] == 0.0)
        others = got[np.arange(12) != 3]
        for side in (0, 1):  # delta, vega, rho and theta of a side are live exactly where some path exercises it
            live = others[:, 20 + side] > 0.0
            assert live.any() and np.array_equal((others[:, [side, 2 + side, 4 + side, 6 + side]] != 0.0).all(axis=1), live)
        assert np.all(got[3, [2, 3, 12, 13]] == 0.0)


@pytest.mark.parametrize("flag", [0, REPLAY])
def test_basket_greeks_single_path_has_zero_stderr(flag) -> None:
    for norm in (0, 1):
        got, _ = _greeks(cases.contracts(4, 12), 4, 4, 1, flag, norm, 0)
        assert not np.isnan(got).any()
        assert np.all(got[:, _stderr_cols(4)] == 0.0)


@pytest.mark.parametrize("flag", [0, REPLAY])
def test_basket_greeks_identical_assets_at_full_correlation(flag) -> None:
    """A = 2, rho = 1, the same asset twice: the matrix is singular, so the correlation columns (and sxc) may be
    anything; every other column is finite and the two assets' deltas and vegas are one value."""
    A, n = 2, 14
    c = np.array([[100.0, 1.0, 0.03, 1.0, 100.0, 100.0, 0.01, 0.01, 0.3, 0.3],
                  [90.0, 0.5, 0.01, 1.0, 80.0, 80.0, 0.0, 0.0, 0.5, 0.5]])
    rest = [k for k in range(2 * n + 4) if k not in (n - 2, n - 1, 2 * n - 2, 2 * n - 1)]
    for T, P in DEGENERATE_SHAPES:
        got, sums = _greeks(c, A, T, P, flag, 1, 0)
        assert np.isfinite(got[:, rest]).all() and np.isfinite(sums[:, :2]).all()
        assert np.all(got[:, :4 * A + 4] != 0.0)
        for first in (0, 2, 4, 6, n, n + 2, n + 4, n + 6):
            assert_rows_equal(got[:, first + 1], got[:, first], f"columns {first + 1} and {first}")


# --------------------------------------------------------------------------- 6. the float64 reference
@pytest.mark.parametrize("math", ["portable", "hw"])
@pytest.mark.parametrize("A,T,P,norm,B", cases.REFERENCE_CASES)
def test_basket_greeks_against_the_float64_reference(A, T, P, norm, B, math) -> None:
    """Every Greek and both prices within cases.ALLOWED_SHARE = 4.8e-3 of the column's own standard error (the
    reference's) of the independent float64 reference, on Sobol-drawn contracts that all pass
    basket_reference.exercise_count_ok.  The share is four times what the float32 restatement in portable math (which
    the kernel equals up to P 2^-52, test 1) measures against the same reference on the CPU: 1.11e-3, asserted by
    tests/test_basket_greeks_reference.py::test_restatement_against_the_reference; the factor covers hardware math
    and an exercise indicator that flips at the strike.  The rho columns first give up the float32 rounding of the
    constant T K df they are multiples of (cases.rho_constant_bound).  The standard errors themselves lie within
    2 ALLOWED_SHARE relative (the error of a root-mean-square against that of a mean)."""
    _oracle.build()
    rows = cases.sobol_rows(_oracle, A, B)
    full = br.reference(_oracle, rows, A, T, P, SEED, ORD0, normalize=bool(norm))
    assert br.exercise_count_ok(full.doubt, P), full.doubt
    ref, ref_sums = gr.greeks(_oracle, rows, A, T, P, SEED, ORD0, normalize=bool(norm))
    eps = br.HW if math == "hw" else br.PORTABLE
    bound = br.reference(_oracle, rows, A, T, P, SEED, ORD0, normalize=bool(norm), eps=eps)
    np.testing.assert_allclose(ref_sums[:, 0], bound.tot, rtol=1e-12, atol=0)
    # every launch the ledger counts for the row in this math: the mode the shape selects and forced replay beside lds
    runs = [r for r in inst.pricing_runs_of("basket greeks", (A, T, P, norm, B)) if r.math == math]
    assert runs and all(r.normalize == bool(norm) for r in runs)
    for run in runs:
        flags = (_lib.MATH_HW if math == "hw" else 0) | (REPLAY if run.force_replay else 0)
        assert _name(A, T, P, flags, norm) == run.name
        got, sums = _greeks(rows, A, T, P, flags, norm)
        assert not np.isnan(got).any() and not np.isnan(sums).any()
        shares = cases.shares_of_stderr(got, ref, rows, A)
        col = max(shares, key=shares.get)
        print(f"A {A} T {T} P {P} norm {norm} {math} {run.name}: largest share of a standard error {shares[col]:.3e} "
              f"(column {col}); allowed {cases.ALLOWED_SHARE:.3e}")
        assert shares[col] <= cases.ALLOWED_SHARE, shares
        for col in gr.mean_columns(A):
            se = gr.stderr_column(A, col)
            if col in (4 * A, 4 * A + 1):  # a constant column's error is rounding noise in both
                live = ref[:, se] > 1e-9 * np.abs(ref[:, col])
            else:
                live = np.ones(B, dtype=bool)
            np.testing.assert_allclose(got[live, se], ref[live, se], rtol=2 * cases.ALLOWED_SHARE, atol=0, err_msg=str(se))
        # the terminal sums within basket_reference's a-priori bound, the other two relative to the sums of magnitudes
        assert br.share_used(sums[:, 0], bound.tot, bound.tot_bound) < 1.0
        if norm:
            scale = np.abs(ref_sums[:, 0]) * (1.0 + np.abs(np.log(bound.xT / rows[:, 4:4 + A, None])).max(axis=2))
            assert np.all(np.abs(sums[:, 1] - ref_sums[:, 1]) <= 1e-4 * scale)


# --------------------------------------------------------------------------- 7. hardware math
@pytest.mark.parametrize("norm", [0, 1])
def test_basket_greeks_hw_math_close_to_portable(norm) -> None:
    """As test_basket_price_hw_math_close_to_portable: per column the batch norm-relative distance from the portable
    restatement, the project's 1e-5 for hardware-transcendental f32 runs.  Unlike a price, a Greek jumps where the
    exercise indicator flips, so a path whose basket lies within 2^-18 K of the strike (four times the 1e-6 the two
    maths' terminal values differ by) may add its whole term to the difference: that allowance is taken from the
    restatement's own terms before the kernel's output is looked at."""
    A, T, P, B = 4, 16, 4096, 32
    c = cases.contracts(A, B)
    x, _ = _terminal(A, T, P, B)
    portable, psums = _greeks(c, A, T, P, 0, norm)
    r = rs.restate(_oracle, c, A, x, norm, psums)
    want, t = r["cols"], r["t"].astype(np.float64)
    k = r["consts"]
    bs = np.zeros((B, P), dtype=f32)
    for i in range(A):
        bs = bs + x[:, i] * k["s"][:, i, None]
    doubt = np.abs(k["K"][:, None] - bs * k["wA"]) <= 2.0 ** -18 * k["K"][:, None]
    got, got_sums = _greeks(c, A, T, P, _lib.MATH_HW, norm)
    assert not np.isnan(got).any() and not np.isnan(got_sums).any()
    print(f"paths within 2^-18 K of the strike: {int(doubt.sum())} of {B * P}")
    n = 4 * A + 6
    for term in range(0, 4 * A + 6, 1):
        col, _ = rs.term_columns(A, term)
        pair = term + A if term < 4 * A and (term // A) % 2 == 0 else term - A if term < 4 * A else term ^ 1
        flips = ((np.abs(t[term]) + np.abs(t[pair])) * doubt).sum(axis=1) / P
        dist = float(np.linalg.norm(got[:, col] - want[:, col]))
        bound = 1e-5 * float(np.linalg.norm(want[:, col])) + float(np.linalg.norm(flips))
        print(f"col {col}: batch norm distance / bound {dist / bound:.3f} (flip allowance {np.linalg.norm(flips):.3e})")
        assert dist <= bound, col
    for col in (2 * n, 2 * n + 1):  # the prices: the price test's bound as it stands
        rel = float(np.linalg.norm(got[:, col] - want[:, col]) / np.linalg.norm(want[:, col]))
        assert rel < 1e-5, col
    assert not np.array_equal(got[:, 0], portable[:, 0])


# --------------------------------------------------------------------------- 8. Python API
def test_basket_greeks_python_api() -> None:
    A, T, N, M, B = 4, 16, 64, 64, 12
    n = 4 * A + 6
    c = cases.contracts(A, B)
    cd = torch.tensor(c, dtype=torch.float64, device=DEV)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="portable")
    res = basket_greeks(cd, cfg, ordinal0=ORD0)
    assert isinstance(res, BasketGreeks)
    torch.cuda.synchronize()
    want, want_sums = _got(A, T, N * M, 1, B)
    assert res.block.shape == (B, 8 * A + 16) and res.block.dtype == torch.float64 and res.block.is_cuda
    assert_rows_equal(res.block.cpu().numpy(), want, "basket_greeks vs the C call")
    for q, name in enumerate(("terminal_sum", "sum_xl", "sum_xc")):
        assert getattr(res, name).shape == (B, A)
        assert_rows_equal(getattr(res, name).cpu().numpy(), want_sums[:, q], name)
    lo, hi = res.block.data_ptr(), res.block.data_ptr() + res.block.numel() * 8
    for j, name in enumerate(("delta_put", "delta_call", "vega_put", "vega_call")):
        for suffix, base in (("", 0), ("_stderr", n)):
            t = getattr(res, name + suffix)
            assert t.shape == (B, A) and lo <= t.data_ptr() < hi, name
            assert_rows_equal(t.cpu().numpy(), want[:, base + j * A:base + (j + 1) * A], name + suffix)
    for j, name in enumerate(("rho_put", "rho_call", "theta_put", "theta_call", "correlation_put", "correlation_call")):
        for suffix, base in (("", 0), ("_stderr", n)):
            t = getattr(res, name + suffix)
            assert t.shape == (B,) and lo <= t.data_ptr() < hi, name
            assert_rows_equal(t.cpu().numpy(), want[:, base + 4 * A + j], name + suffix)
    for j, name in enumerate(("put", "call", "put_stderr", "call_stderr")):
        assert_rows_equal(getattr(res, name).cpu().numpy(), want[:, 2 * n + j], name)
    # replay: the same bits; n_paths: any positive count; RAW and hw through the configuration
    assert_rows_equal(basket_greeks(cd, cfg, ordinal0=ORD0, replay=True).block.cpu().numpy(), want, "replay=True")
    odd = basket_greeks(cd, cfg, ordinal0=ORD0, n_paths=693)
    assert_rows_equal(odd.block.cpu().numpy(), _greeks(c, A, T, 693, 0, 1)[0], "n_paths = 693")
    raw_cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="portable",
                           normalize=False)
    assert_rows_equal(basket_greeks(cd, raw_cfg, ordinal0=ORD0).block.cpu().numpy(), _greeks(c, A, T, N * M, 0, 0)[0], "RAW")
    hw_cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="hw")
    hw = basket_greeks(cd, hw_cfg, ordinal0=ORD0).block.cpu().numpy()
    assert_rows_equal(hw, _greeks(c, A, T, N * M, _lib.MATH_HW, 1)[0], 'math="hw" vs SMC_MATH_HW')
    assert not np.array_equal(hw[:, 0], want[:, 0])
    # the empty batch: empty tensors, no launch
    empty = basket_greeks(cd[:0], cfg)
    assert empty.block.shape == (0, 8 * A + 16) and empty.delta_put.shape == (0, A) and empty.sum_xc.shape == (0, A)
    for bad in (cd[:, :5], cd.to(torch.float32), cd.reshape(-1), cd.cpu()):
        with pytest.raises(ValueError):
            basket_greeks(bad, cfg)
    with pytest.raises(ValueError):
        basket_greeks(cd, cfg, n_paths=0)


def test_basket_engine_greeks() -> None:
    cfg = BasketConfig(n_assets=3, timesteps=8, network_size=64, batches_per_mc_run=32, mc_seed=SEED, math="portable")
    eng = BasketEngine(cfg, 16, device=torch.device(DEV))
    eng.set_position(0, 0)
    eng.enqueue_step()
    got = eng.greeks()
    want = basket_greeks(eng.buffers.contracts, cfg)
    price = eng.price()
    torch.cuda.synchronize()
    assert got.block.shape == (16, 40) and not bool(torch.isnan(got.block).any())
    assert_rows_equal(got.block.cpu().numpy(), want.block.cpu().numpy(), "BasketEngine.greeks vs basket_greeks")
    assert_rows_equal(got.put.cpu().numpy(), price.basket_put.cpu().numpy(), "the put vs BasketEngine.price")
    assert_rows_equal(got.terminal_sum.cpu().numpy(), eng.terminal_sum.cpu().numpy(), "terminal sums of the step")
    other = eng.greeks(eng.buffers.contracts[:4], ordinal0=2, n_paths=100)
    assert_rows_equal(other.block.cpu().numpy(),
                      basket_greeks(eng.buffers.contracts[:4], cfg, ordinal0=2, n_paths=100).block.cpu().numpy(), "overrides")


def test_basket_greeks_call_is_capturable() -> None:
    A, T, P, B = 4, 16, 4096, 12
    eager, eager_sums = _got(A, T, P, 1, B)
    cd = torch.tensor(cases.contracts(A, B), dtype=torch.float64, device=DEV)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=64, mc_seed=SEED, math="portable")
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        res = basket_greeks(cd, cfg, ordinal0=ORD0)
    res.block.fill_(float("nan"))  # capturing launched nothing; an element the replay leaves unwritten shows
    for t in (res.terminal_sum, res.sum_xl, res.sum_xc):
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(res.block.cpu().numpy(), eager, "replayed graph vs eager")
    assert_rows_equal(torch.stack([res.terminal_sum, res.sum_xl, res.sum_xc], dim=1).cpu().numpy(), eager_sums,
                      "replayed graph vs eager, sums")
