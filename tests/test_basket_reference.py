"""The basket engine against the independent float64 reference of tests/helpers/basket_reference.py, on the CPU: the
oracle's kernel mode (oracle_basket_kernel, which tests/test_gpu_basket.py shows equal to the kernels bit for bit in
portable math) stands in for the kernels, and every stored path element, terminal sum, target and price column has to
lie within the a-priori bound the helper derives.  tests/test_gpu_basket_reference.py holds the kernels themselves to
the same reference.

The price columns have no kernel-mode restatement in the oracle: _kernel_price_columns restates the header's table in
numpy float32 from the oracle's terminal values (as tests/test_gpu_basket_price.py does for its bit-level checks).

The sensitivity test is what gives the bounds their meaning: each wrong reading of the engine listed there, put in
the reference's place, has to leave the bound somewhere.  The reference itself is held to closed forms of its own."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from spectralmc_amd.basket import BasketConfig, default_basket_bounds
from tests.helpers import basket_reference as br

SEED = 7
ORD0 = 3
N = 64
f32 = np.float32


def _sobol_rows(oracle, A: int, n: int = 4) -> np.ndarray:
    lo, hi = BasketConfig(n_assets=A, network_size=N, batches_per_mc_run=32).arrays()
    return oracle.sobol_contracts(SEED, 0, n, lo, hi)


def _kernel_price_columns(oracle, rows: np.ndarray, A: int, x: np.ndarray, tot: np.ndarray, normalize: bool) -> np.ndarray:
    """smc_basket_price's 18 columns as include/spectralmc_hip.h states them, per path in float32 (asset order, the
    portable exp), from raw terminal values x [B, A, P] f32 and terminal sums [B, A] f64."""
    B, _, P = x.shape
    assert x.dtype == f32
    K, Tm, r, _, X0, d, _ = br.fields(rows, A)
    Kf, Tf = K.astype(f32)[:, None], Tm.astype(f32)
    df = oracle.exp_n((-r).astype(f32) * Tf)[:, None]
    F = X0.astype(f32) * oracle.exp_n(((r[:, None] - d).astype(f32) * Tf[:, None]).ravel()).reshape(B, A)
    s = F / (tot / float(P)).astype(f32) if normalize else np.ones((B, A), dtype=f32)
    xs = x * s[:, :, None]
    bs, fs = np.zeros((B, P), dtype=f32), np.zeros(B, dtype=f32)
    for i in range(A):
        bs, fs = bs + xs[:, i], fs + F[:, i]
    wA = f32(1.0 / A)
    under = [bs * wA, xs.max(axis=1), xs.min(axis=1)]
    assert all(u.dtype == f32 for u in under) and df.dtype == f32

    def pay(diff: np.ndarray) -> np.ndarray:
        return (df * np.maximum(diff, f32(0))).astype(np.float64)

    v = [pay(sign * (Kf - u)) for u in under for sign in (f32(1), f32(-1))]
    cols = np.zeros((B, 18))
    for k in range(6):
        cols[:, k] = v[k].sum(axis=1) / P
        if P > 1:
            cols[:, 6 + k] = np.sqrt(np.maximum((v[k] * v[k]).sum(axis=1) - P * cols[:, k] ** 2, 0.0) / (P - 1) / P)
    for k in range(3):
        cols[:, 12 + k] = under[k].astype(np.float64).sum(axis=1) / P
    cols[:, 15] = (under[0] < Kf).sum(axis=1) / P
    Fb = (fs * wA)[:, None]
    cols[:, 16], cols[:, 17] = pay(Kf - Fb)[:, 0], pay(Fb - Kf)[:, 0]
    return cols


def _compare(oracle, rows: np.ndarray, A: int, T: int, M: int, label: str) -> dict[str, float]:
    """Every output of the oracle's kernel mode against the reference: the largest share of the bound used, by output."""
    P = N * M
    paths, tot, tg = oracle.basket_kernel(rows, A, T, N, M, SEED, ordinal0=ORD0, want_paths=True)
    ref = br.reference(oracle, rows, A, T, P, SEED, ORD0, N=N, M=M, keep_paths=True)
    raw = br.reference(oracle, rows, A, T, P, SEED, ORD0, normalize=False)
    assert br.exercise_count_ok(ref.doubt, P) and br.exercise_count_ok(raw.doubt, P), (label, ref.doubt, raw.doubt)
    xT = np.ascontiguousarray(paths[:, :, -1, :])
    used = {"paths": br.share_used(paths, ref.x, ref.paths_bound),
            "sums": br.share_used(tot, ref.tot, ref.tot_bound),
            "targets": br.complex_share_used(tg, ref.targets, ref.targets_bound),
            "price": br.share_used(_kernel_price_columns(oracle, rows, A, xT, tot, True), ref.cols, ref.cols_bound),
            "price raw": br.share_used(_kernel_price_columns(oracle, rows, A, xT, tot, False), raw.cols, raw.cols_bound)}
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
          + f"; last-step path bound {ref.relT.min():.2e} .. {ref.relT.max():.2e}")
    return used


@pytest.mark.parametrize("M", [32, 64])  # P = 2048, and 4096: the second chunk's groups
@pytest.mark.parametrize("T", [1, 3, 5, 16])
@pytest.mark.parametrize("A", [1, 2, 3, 4, 5, 7, 8])
def test_kernel_mode_within_the_bound_on_sobol_contracts(oracle, A, T, M) -> None:
    used = _compare(oracle, _sobol_rows(oracle, A), A, T, M, f"A {A} T {T} P {N * M}")
    assert max(used.values()) < 1.0, used


@pytest.mark.parametrize("A,T,M", [(1, 3, 32), (2, 16, 32), (4, 5, 64), (8, 3, 32), (7, 16, 32)])
def test_kernel_mode_within_the_bound_on_hand_built_rows(oracle, A, T, M) -> None:
    hand = br.hand_built_rows(A)
    if A == 8:
        assert hand["rho lower bound"][3] == default_basket_bounds(8)["rho"][0]
    for name, row in hand.items():
        used = _compare(oracle, row[None, :], A, T, M, f"A {A} T {T} P {N * M} {name}")
        assert max(used.values()) < 1.0, (name, used)


# ---- sensitivity: wrong references leave the bound ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stage(A: int, T: int, M: int):
    """The pieces of one case (Sobol rows and the hand-built ones), for the mutants to recombine."""
    import oracle  # noqa: PLC0415

    oracle.build()
    rows = np.concatenate([_sobol_rows(oracle, A), np.stack(list(br.hand_built_rows(A).values()))])
    P = N * M
    z, rad = br.drivers(br.stream_words(oracle, rows.shape[0], A, T, P, SEED, ORD0))
    kp, ktot, ktg = oracle.basket_kernel(rows, A, T, N, M, SEED, ordinal0=ORD0, want_paths=True)
    xT = np.ascontiguousarray(kp[:, :, -1, :])
    kcols = _kernel_price_columns(oracle, rows, A, xT, ktot, True)
    return rows, z, rad, kp, ktg, kcols


def _paths_rejected(A: int, T: int, M: int, **wrong) -> float:
    """The share of its own bound by which the kernel mode misses a reference with one thing wrong."""
    rows, z, rad, kp, _, _ = _stage(A, T, M)
    rows = wrong.pop("rows", rows)
    slots = wrong.pop("slots", list(range(A)))
    x, rel = br.paths(rows, A, T, z[:, slots], rad[:, slots], br.PORTABLE, **wrong)
    return br.share_used(kp, x, x * rel)


def _outputs_rejected(A: int, T: int, M: int, wrong: str) -> float:
    rows, z, rad, _, ktg, kcols = _stage(A, T, M)
    x, rel = br.paths(rows, A, T, z[:, :A], rad[:, :A], br.PORTABLE)
    good = br.outputs(rows, A, x, rel, N, M, True)
    B = rows.shape[0]
    if wrong == "reshape":  # path p read as row p % M, column p // M
        v, dv = br.payoffs(rows, A, good.u[:1], good.du[:1])
        tg, _ = br.targets(v[0].reshape(B, N, M).transpose(0, 2, 1).reshape(B, -1), dv[0], N, M)
        return br.complex_share_used(ktg, tg, good.targets_bound)
    if wrong == "best and worst":
        swap = [0, 1, 4, 5, 2, 3, 6, 7, 10, 11, 8, 9, 12, 14, 13, 15, 16, 17]
        return br.share_used(kcols, good.cols[:, swap], good.cols_bound[:, swap])
    if wrong == "weights":  # 1 / (A + 1)
        u = good.u.copy()
        u[0] *= A / (A + 1.0)
        cols, bound, _ = br.price_columns(rows, A, u, good.du)
        v, dv = br.payoffs(rows, A, u[:1], good.du[:1])
        tg, tb = br.targets(v[0], dv[0], N, M)
        return min(br.share_used(kcols[:, [0, 1, 12]], cols[:, [0, 1, 12]], bound[:, [0, 1, 12]]),
                   br.complex_share_used(ktg, tg, tb))
    assert wrong == "forward"  # asset i scaled to the forward of asset i - 1
    F, eF, _, _ = br.forwards(rows, A)
    u, du = br.underlyings(*br.scaled(good.xT, good.relT, good.tot, good.tot_bound, True, np.roll(F, 1, axis=1),
                                      np.roll(eF, 1, axis=1)))
    cols, bound, _ = br.price_columns(rows, A, u, du)
    return br.share_used(kcols[:, :16], cols[:, :16], bound[:, :16])


def test_wrong_references_leave_the_bound() -> None:
    A, T, M = 3, 16, 32  # odd A: a discarded sine; T = 16: the drift mutant's case
    rows, z, _, _, _, _ = _stage(A, T, M)
    _, Tm, r, rho, _, d, v = br.fields(rows, A)
    dt = Tm / T
    swapped = rows.copy()
    swapped[:, 4 + A:4 + 2 * A], swapped[:, 4 + 2 * A:] = rows[:, 4 + 2 * A:], rows[:, 4 + A:4 + 2 * A]
    assert z.shape[1] == A + 1
    good = _paths_rejected(A, T, M)
    missed = {
        "L transposed": _paths_rejected(A, T, M, L=np.stack([br.factor(A, rh).T for rh in rho])),
        "drivers of a pair exchanged": _paths_rejected(A, T, M, slots=[1, 0, 3]),
        "odd A one slot later": _paths_rejected(A, T, M, slots=[1, 2, 3]),
        "d and v exchanged": _paths_rejected(A, T, M, rows=swapped),
        "no -v^2/2": _paths_rejected(A, T, M, drift=r[:, None] - d),
        "drift off by 1e-6 per step": _paths_rejected(A, T, M, drift=r[:, None] - d - 0.5 * v * v + 1e-6 / dt[:, None]),
        "dt = T / (steps + 1)": _paths_rejected(A, T, M, dt=Tm / (T + 1)),
        "(M, N) reshape transposed": _outputs_rejected(A, T, M, "reshape"),
        "best-of and worst-of exchanged": _outputs_rejected(A, T, M, "best and worst"),
        "weights 1 / (A + 1)": _outputs_rejected(A, T, M, "weights"),
        "forward of a neighbouring asset": _outputs_rejected(A, T, M, "forward"),
    }
    print(f"the reference: {good:.3f} of its bound; the wrong ones: " + ", ".join(f"{k} {v:.3g}" for k, v in missed.items()))
    assert good < 1.0
    survivors = [k for k, v in missed.items() if not v > 1.0]
    assert not survivors, survivors


def test_wrong_references_leave_the_bound_at_even_assets() -> None:
    """The same at A = 4, T = 5, P = 4096 for the mutants that do not need an odd A or T = 16."""
    A, T, M = 4, 5, 64
    rows, _, _, _, _, _ = _stage(A, T, M)
    _, Tm, r, rho, _, d, _ = br.fields(rows, A)
    missed = {
        "L transposed": _paths_rejected(A, T, M, L=np.stack([br.factor(A, rh).T for rh in rho])),
        "drivers of a pair exchanged": _paths_rejected(A, T, M, slots=[1, 0, 3, 2]),
        "no -v^2/2": _paths_rejected(A, T, M, drift=r[:, None] - d),
        "dt = T / (steps + 1)": _paths_rejected(A, T, M, dt=Tm / (T + 1)),
        "(M, N) reshape transposed": _outputs_rejected(A, T, M, "reshape"),
        "best-of and worst-of exchanged": _outputs_rejected(A, T, M, "best and worst"),
        "weights 1 / (A + 1)": _outputs_rejected(A, T, M, "weights"),
        "forward of a neighbouring asset": _outputs_rejected(A, T, M, "forward"),
    }
    print(", ".join(f"{k} {v:.3g}" for k, v in missed.items()))
    assert _paths_rejected(A, T, M) < 1.0
    assert all(v > 1.0 for v in missed.values()), missed


# ---- the reference against closed forms of its own -----------------------------------------------------------------
def test_stream_words_array_form(oracle) -> None:
    w = oracle.stream_u32_groups(SEED, 5, 3, 4, 24)
    for k in range(4):
        np.testing.assert_array_equal(w[k], oracle.stream_u32(SEED, 5, 3 + k, 24))


def test_reference_single_asset_is_blacks_put(oracle) -> None:
    rng = np.random.default_rng(11)
    B, P = 8, 65536
    x0 = rng.uniform(50, 150, B)
    rows = np.stack([x0 * rng.uniform(0.8, 1.25, B), rng.uniform(0.25, 2, B), rng.uniform(-0.02, 0.08, B),
                     np.zeros(B), x0, rng.uniform(0, 0.04, B), rng.uniform(0.1, 0.6, B)], axis=1)
    ref = br.reference(oracle, rows, 1, 16, P, SEED, 0)
    black = np.array([oracle.black_put(c[4], c[0], c[1], c[2], c[5], c[6]) for c in rows.tolist()])
    z = np.abs(ref.cols[:, 0] - black) / ref.cols[:, 6]
    print(f"|put - Black| / stderr: {np.round(z, 2).tolist()}")
    assert np.all(ref.cols[:, 0] > 0.0) and np.all(z <= 4.0)
    # one asset: basket, best and worst are the asset
    np.testing.assert_allclose(ref.cols[:, [2, 3, 8, 9, 13]], ref.cols[:, [0, 1, 6, 7, 12]], rtol=1e-12)
    np.testing.assert_allclose(ref.cols[:, [4, 5, 10, 11, 14]], ref.cols[:, [0, 1, 6, 7, 12]], rtol=1e-12)


@pytest.mark.parametrize("A,rho", [(4, 0.6), (3, -0.3), (8, 0.9), (2, 1.0)])
def test_reference_drivers_have_the_correlation(oracle, A, rho) -> None:
    P = 65536
    z, _ = br.drivers(br.stream_words(oracle, 1, A, 1, P, SEED, ORD0))
    z = z[0, :A, 0, :]
    tol = 4.0 / np.sqrt(P)
    assert np.all(np.abs(np.corrcoef(z) - np.eye(A)) <= tol) if A > 1 else True
    assert np.all(np.abs(z.mean(axis=1)) <= tol) and np.all(np.abs(z.var(axis=1) - 1.0) <= 2 * tol)
    L = br.factor(A, rho)
    C = (1.0 - rho) * np.eye(A) + rho * np.ones((A, A))
    np.testing.assert_allclose(L @ L.T, C, atol=1e-14)
    assert np.all(np.triu(L, 1) == 0.0)
    got = np.corrcoef(L @ z)
    print(f"A {A} rho {rho}: largest |corr - C| {np.abs(got - C).max():.4f} (bound {tol:.4f})")
    assert np.all(np.abs(got - C) <= tol)
