"""basket_general_kernel (smc_basket_price_general) on the device, every output into NaN-poisoned buffers:
against the independent float64 reference of tests/helpers/basket_general_reference.py in portable and SMC_MATH_HW
math (all 18 columns and the terminal sums within the helper's a-priori bound, which is computed, with the
exercise-count condition, before the kernel's output is looked at); the bit-for-bit relations the header states
(an all-rho matrix is no matrix, equal weights are smc_basket_price, stride 0 is the row repeated, lds is replay,
run to run, any split, ordinal on host or device); the Margrabe exchange option; the orderings and the forward
parity of convex weights; and the Python surface.  tests/test_basket_general_reference.py shows on the CPU that wrong
readings of the weights and of the packed triangle leave that bound."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.basket import BasketConfig, BasketEngine, basket_price, pack_correlation
from tests.helpers import basket_general_cases as cases
from tests.helpers import basket_general_reference as gr
from tests.helpers import basket_reference as br
from tests.helpers import instantiations as inst
from tests.helpers import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, ORD0 = cases.SEED, cases.ORD0
MATHS = {"portable": (br.PORTABLE, 0), "hw": (br.HW, _lib.MATH_HW)}
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
RAINBOW = [2, 3, 4, 5, 8, 9, 10, 11, 13, 14]


def _name(A: int, T: int, P: int, flags: int, norm: int) -> str:
    return _lib.lib().smc_basket_price_general_kernel(A, T, P, flags, norm).decode()


def _dev(a: np.ndarray | None) -> torch.Tensor | None:
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _general(rows: np.ndarray, A: int, T: int, P: int, flags: int, norm: int, *, w: np.ndarray | None = None,
             ws: int | None = None, tri: np.ndarray | None = None, cs: int | None = None, ordinal0: int = ORD0,
             seed: int = SEED, ordinal_dev: torch.Tensor | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(block [B, 18], terminal sums [B, A]) of one C call; w [A] or [B, A], tri [n] or [B, n] (strides default to 0
    for a single row, to the row length otherwise)."""
    B = rows.shape[0]
    cd, wd, td = _dev(rows), _dev(w), _dev(tri)
    ws = (0 if w is None or w.ndim == 1 else w.shape[1]) if ws is None else ws
    cs = (0 if tri is None or tri.ndim == 1 else tri.shape[1]) if cs is None else cs
    out = poisoned((B, _lib.BASKET_PRICE_COLS), torch.float64, DEV)
    tsum = poisoned((B, A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price_general(
        _lib.ptr(cd), _lib.ptr(wd), ws, _lib.ptr(td), cs, B, A, T, P, seed, _lib.ptr(ordinal_dev), ordinal0, flags,
        norm, _lib.ptr(out), _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy(), tsum.cpu().numpy()
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    return got


def _price(rows: np.ndarray, A: int, T: int, P: int, flags: int, norm: int,
           ordinal0: int = ORD0) -> tuple[np.ndarray, np.ndarray]:
    cd = _dev(rows)
    out = poisoned((rows.shape[0], _lib.BASKET_PRICE_COLS), torch.float64, DEV)
    tsum = poisoned((rows.shape[0], A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price(_lib.ptr(cd), rows.shape[0], A, T, P, SEED, None, ordinal0, flags, norm,
                                           _lib.ptr(out), _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tsum.cpu().numpy()


def _check(got: tuple[np.ndarray, np.ndarray], ref: gr.GeneralRef, label: str) -> None:
    cols, tsum = got
    P = ref.xT.shape[-1]
    used = {"sums": br.share_used(tsum, ref.tot, ref.tot_bound)}
    for name, sel in (("prices", slice(0, 6)), ("stderr", slice(6, 12)), ("means", slice(12, 15)),
                      ("exercise", slice(15, 16)), ("intrinsic", slice(16, 18))):
        used[name] = br.share_used(cols[:, sel], ref.cols[:, sel], ref.cols_bound[:, sel])
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) <= 1.0, (label, used)  # the exercise share is a count: it may use its whole tolerance
    assert max(v for k, v in used.items() if k != "exercise") < 1.0, (label, used)
    if P == 1:
        assert np.all(cols[:, 6:12] == 0.0), label


@functools.lru_cache(maxsize=None)
def _drawn(A: int, B: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    return cases.drawn_case(_oracle, A, B)


def _against_reference(rows, w, C, A, T, P, norm, label) -> None:
    tri = cases.pack(C)
    refs = {}
    # every launch the ledger counts for the row: both maths, the mode the shape selects and forced replay beside lds
    for run in inst.pricing_runs_of("basket general", (A, T, P, norm, rows.shape[0])):
        eps, hw = MATHS[run.math]
        if run.math not in refs:
            refs[run.math] = gr.reference(_oracle, rows, A, T, P, SEED, ORD0, weights=w, corr=C, normalize=bool(norm), eps=eps)
            assert br.exercise_count_ok(refs[run.math].doubt, P), refs[run.math].doubt  # before the kernel's output
        flags = hw | (_lib.PRICE_REPLAY if run.force_replay else 0)
        assert _name(A, T, P, flags, norm) == run.name and run.normalize == bool(norm)
        _check(_general(rows, A, T, P, flags, norm, w=w, tri=tri), refs[run.math], f"{label} {run.math} {run.name}")


# ---- against the float64 reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("A,T,P,norm,B", cases.CASES)
def test_general_kernel_columns_and_sums_against_the_reference(A, T, P, norm, B) -> None:
    want = "raw" if not norm else ("replay" if A * ((P + 3) // 4 * 4) * 4 + 2112 > 144 * 1024 else "lds")
    assert _name(A, T, P, 0, norm) == f"basket_general_kernel({want})"
    assert (A, P, want) != (2, 65536, "lds") and (A, P, want) != (4, 4096, "replay")
    rows, w, C = _drawn(A, B)
    _against_reference(rows, w, C, A, T, P, norm, f"general A {A} T {T} P {P}")


def test_general_kernel_spread_against_the_reference() -> None:
    """A = 2, weights (1, -1), K = 0: partial sums that change sign, a strike of zero."""
    rows, w, C = cases.spread_case(_oracle)
    _against_reference(rows, w, C, 2, 4, 2049, NORM, "spread")
    _against_reference(rows, w, C, 2, 4, 2049, RAW, "spread RAW")


# ---- the bit-for-bit relations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", range(1, 9))
def test_all_rho_matrix_is_no_matrix_and_equal_weights_are_basket_price(A) -> None:
    T, P, B = 3, 2049, 4
    rows, w, _ = _drawn(A, B)
    n = A * (A - 1) // 2
    tri = np.repeat(rows[:, 3:4], n, axis=1)  # every entry the row's rho
    for hw in (0, _lib.MATH_HW):
        for norm in (NORM, RAW):
            # (a) with the drawn weights
            a0 = _general(rows, A, T, P, hw, norm, w=w)
            a1 = _general(rows, A, T, P, hw, norm, w=w, tri=tri, cs=n)
            np.testing.assert_array_equal(a0[0], a1[0])
            np.testing.assert_array_equal(a0[1], a1[1])
            # (b) equal weights, NULL or explicit, no matrix or the all-rho one
            price = _price(rows, A, T, P, hw, norm)
            for kw in ({}, {"w": np.full(A, 1.0 / A)}, {"w": np.full((B, A), 1.0 / A), "tri": tri, "cs": n}):
                g = _general(rows, A, T, P, hw, norm, **kw)
                np.testing.assert_array_equal(g[1], price[1])
                np.testing.assert_array_equal(g[0][:, RAINBOW], price[0][:, RAINBOW])
                if A in (1, 2, 4, 8):  # f32(1 / A) is a power of two: the weighted sum is the scaled sum
                    np.testing.assert_array_equal(g[0], price[0])
            # the drawn weights do change the basket
            assert not np.array_equal(a0[0][:, 12], price[0][:, 12]) or A == 1


def test_whole_block_is_basket_price_in_lds_and_replay() -> None:
    """The whole block at A = 2, 4, 8 and the rainbow columns at A = 3, in the lds and the replay kernels, over two
    chunks and a ragged tail."""
    T, P, B = 4, 4099, 3
    for A in (2, 3, 4, 8):
        rows = _drawn(A, 6)[0][:B]
        for flags in (0, _lib.PRICE_REPLAY, _lib.MATH_HW, _lib.MATH_HW | _lib.PRICE_REPLAY):
            price = _price(rows, A, T, P, flags, NORM)
            g = _general(rows, A, T, P, flags, NORM)
            np.testing.assert_array_equal(g[1], price[1])
            cols = RAINBOW if A == 3 else list(range(18))
            np.testing.assert_array_equal(g[0][:, cols], price[0][:, cols])


@pytest.mark.parametrize("A", [2, 5])
def test_stride_zero_is_the_row_repeated(A) -> None:
    T, P, B = 3, 1000, 5
    rows, w, C = _drawn(A, 6)
    rows, tri = rows[:B], cases.pack(C)
    n = tri.shape[1]
    for hw in (0, _lib.MATH_HW):
        shared = _general(rows, A, T, P, hw, NORM, w=w[1], tri=tri[2])
        full = _general(rows, A, T, P, hw, NORM, w=np.tile(w[1], (B, 1)), tri=np.tile(tri[2], (B, 1)))
        np.testing.assert_array_equal(shared[0], full[0])
        np.testing.assert_array_equal(shared[1], full[1])
        # padded rows: a stride above the row length
        wp, tp = np.full((B, A + 3), np.nan), np.full((B, n + 2), np.nan)
        wp[:, :A], tp[:, :n] = w[:B], tri[:B]
        packed = _general(rows, A, T, P, hw, NORM, w=w[:B], tri=tri[:B])
        padded = _general(rows, A, T, P, hw, NORM, w=wp, ws=A + 3, tri=tp, cs=n + 2)
        np.testing.assert_array_equal(packed[0], padded[0])
        assert not np.array_equal(packed[0][:, 0], shared[0][:, 0])


def test_lds_is_replay_run_to_run_any_split_and_ordinal_on_the_device() -> None:
    A, T, P, B = 4, 5, 4099, 6
    rows, w, C = _drawn(A, B)
    tri = cases.pack(C)
    for hw in (0, _lib.MATH_HW):
        assert _name(A, T, P, hw, NORM) == "basket_general_kernel(lds)"
        lds = _general(rows, A, T, P, hw, NORM, w=w, tri=tri)
        again = _general(rows, A, T, P, hw, NORM, w=w, tri=tri)
        replay = _general(rows, A, T, P, hw | _lib.PRICE_REPLAY, NORM, w=w, tri=tri)
        for other in (again, replay):
            np.testing.assert_array_equal(lds[0], other[0])
            np.testing.assert_array_equal(lds[1], other[1])
        parts = [_general(rows[s], A, T, P, hw, NORM, w=w[s], tri=tri[s], ordinal0=ORD0 + s.start)
                 for s in (slice(0, 1), slice(1, 4), slice(4, 6))]
        np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), lds[0])
        np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), lds[1])
        od = torch.tensor([ORD0 - 2], dtype=torch.int64, device=DEV)
        on_dev = _general(rows, A, T, P, hw, NORM, w=w, tri=tri, ordinal0=2, ordinal_dev=od)
        np.testing.assert_array_equal(on_dev[0], lds[0])
        other_stream = _general(rows, A, T, P, hw, NORM, w=w, tri=tri, ordinal0=ORD0 + 1)
        assert not np.array_equal(other_stream[0][:, 0], lds[0][:, 0])


# ---- Margrabe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [NORM, RAW], ids=["NORMALIZE", "RAW"])
def test_margrabe_exchange_option_on_the_device(norm) -> None:
    rows = cases.margrabe_rows()
    m = cases.MARGRABE
    want = gr.margrabe(rows)
    w = np.array([1.0, -1.0])
    for math, (_, hw) in MATHS.items():
        modes = {_name(2, m["T"], m["P"], hw, norm): hw}
        if norm:
            modes[_name(2, m["T"], m["P"], hw | _lib.PRICE_REPLAY, norm)] = hw | _lib.PRICE_REPLAY
            assert set(modes) == {"basket_general_kernel(lds)", "basket_general_kernel(replay)"}
        for mode, flags in modes.items():
            cols, _ = _general(rows, 2, m["T"], m["P"], flags, norm, w=w, seed=m["seed"], ordinal0=m["ordinal0"])
            z = np.abs(cols[:, 1] - want) / cols[:, 7]
            print(f"Margrabe {math} {mode}: worst {z.max():.2f} standard errors")
            assert np.all(z < 5.0), (math, mode, z)


# ---- convex weights --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,T,P,norm,B", [c for c in cases.CASES if c[2] <= 4096])
def test_convex_weights_orderings_and_forward_parity(A, T, P, norm, B) -> None:
    """Weights >= 0 that sum to 1.  A path's bk = fl(sum f32(w_i) xs_i) lies within g = (1 + U)^(A + 1) - 1 (relative)
    of a convex combination of its xs_i, so mn (1 - g) <= bk <= mx (1 + g) per path and in the means; a payoff
    df max(+-(K - u), 0) is 1-Lipschitz in u and carries two roundings of its own on either side of an inequality
    (4 U of a payoff that is at most df (mx + K)), which with g (1 + 2 U) <= g + U gives the slack below.
    NORMALIZE: the mean of xs_i over the paths is the kernel's F_i up to the 3 f32 roundings in the lane sums of
    tot_i, the roundings of tot_i / P, of the division and of x_i s_i (U each) and the f64 sums (P 2^-52); the
    kernel's F_i is within the reference's eF_i of the exact forward; the weighted sum adds g."""
    rows, w, C = _drawn(A, B)
    assert np.all(w >= 0.0) and np.allclose(w.sum(axis=1), 1.0, rtol=1e-14)
    U = br.U
    g = (1.0 + U) ** (A + 1) - 1.0
    F, eF, df, _ = br.forwards(rows, A)
    for math, (_, hw) in MATHS.items():
        got, _ = _general(rows, A, T, P, hw, norm, w=w, tri=cases.pack(C))
        assert np.all(got[:, 14] * (1.0 - g) <= got[:, 12]) and np.all(got[:, 12] <= got[:, 13] * (1.0 + g))
        slack = df * (g + 5 * U) * (got[:, 13] + rows[:, 0])
        assert np.all(got[:, 3] + slack >= got[:, 1]) and np.all(got[:, 1] + slack >= got[:, 5])  # calls
        assert np.all(got[:, 4] + slack >= got[:, 0]) and np.all(got[:, 0] + slack >= got[:, 2])  # puts
        assert np.all(got[:, :12] >= 0.0) and np.all(got[:, 15] >= 0.0) and np.all(got[:, 15] <= 1.0)
        if norm:
            bound = (w * F * br.compose(eF, 3 * U, U, U, U, g, P * 2.0 ** -52)).sum(axis=1)
            err = np.abs(got[:, 12] - (w * F).sum(axis=1))
            print(f"mean basket against sum w F, A {A} {math}: share of the bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound)


# ---- the Python surface ----------------------------------------------------------------------------------------------------
def test_basket_price_with_weights_and_correlation_is_the_c_call() -> None:
    A, T, P, B = 4, 5, 1000, 6
    rows, w, C = _drawn(A, B)
    tri = cases.pack(C)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=32, mc_seed=SEED, math="portable")
    cd, wd, Cd, td = _dev(rows), _dev(w), _dev(C), _dev(tri)
    np.testing.assert_array_equal(pack_correlation(Cd).cpu().numpy(), tri)
    per = _general(rows, A, T, P, 0, NORM, w=w, tri=tri)
    shared = _general(rows, A, T, P, 0, NORM, w=w[0], tri=tri[0])
    only_w = _general(rows, A, T, P, 0, NORM, w=w)
    only_c = _general(rows, A, T, P, 0, NORM, tri=tri)
    for want, kw in ((per, dict(weights=wd, correlation=Cd)), (per, dict(weights=wd, correlation=td)),
                     (shared, dict(weights=wd[0].contiguous(), correlation=Cd[0].contiguous())),
                     (shared, dict(weights=wd[0].contiguous(), correlation=td[0].contiguous())),
                     (only_w, dict(weights=wd)), (only_c, dict(correlation=Cd)),
                     (per, dict(weights=wd, correlation=Cd, validate=True))):
        got = basket_price(cd, cfg, ordinal0=ORD0, n_paths=P, **kw)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.block.cpu().numpy(), want[0])
        np.testing.assert_array_equal(got.terminal_sum.cpu().numpy(), want[1])
        np.testing.assert_array_equal(got.mean_basket.cpu().numpy(), want[0][:, 12])
    replay = basket_price(cd, cfg, ordinal0=ORD0, n_paths=P, replay=True, weights=wd, correlation=Cd)
    np.testing.assert_array_equal(replay.block.cpu().numpy(), per[0])
    # validate=True on device tensors
    bad = Cd.clone()
    bad[2] = -0.9
    bad[2].fill_diagonal_(1.0)
    with pytest.raises(ValueError, match="positive definite"):
        basket_price(cd, cfg, n_paths=P, correlation=bad, validate=True)
    with pytest.raises(ValueError, match="finite"):
        basket_price(cd, cfg, n_paths=P, weights=wd * float("inf"), validate=True)
    # without the new arguments: today's call, bit for bit
    plain = basket_price(cd, cfg, ordinal0=ORD0, n_paths=P)
    want = _price(rows, A, T, P, 0, NORM)
    np.testing.assert_array_equal(plain.block.cpu().numpy(), want[0])
    np.testing.assert_array_equal(plain.terminal_sum.cpu().numpy(), want[1])
    # an empty batch
    empty = basket_price(cd[:0], cfg, n_paths=P, weights=wd[0].contiguous(), correlation=Cd[0].contiguous())
    assert empty.block.shape == (0, 18)


def test_engine_price_takes_weights_and_correlation() -> None:
    A, T, N, M, B = 3, 4, 64, 32, 6
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="hw")
    eng = BasketEngine(cfg, B, device=torch.device(DEV))
    eng.set_position(0, 0)
    eng.enqueue_step()
    _, w, C = _drawn(A, B)
    got = eng.price(ordinal0=ORD0, n_paths=693, weights=_dev(w), correlation=_dev(C))
    torch.cuda.synchronize()
    rows = eng.buffers.contracts.cpu().numpy()
    want = _general(rows, A, T, 693, _lib.MATH_HW, NORM, w=w, tri=cases.pack(C))
    np.testing.assert_array_equal(got.block.cpu().numpy(), want[0])
    plain = eng.price(ordinal0=ORD0, n_paths=693)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(plain.block.cpu().numpy(), _price(rows, A, T, 693, _lib.MATH_HW, NORM)[0])


def test_general_call_is_capturable_in_a_graph() -> None:
    A, T, P, B = 4, 5, 1000, 6
    rows, w, C = _drawn(A, B)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=32, mc_seed=SEED, math="hw")
    cd, wd, td = _dev(rows), _dev(w), _dev(cases.pack(C))
    want = _general(rows, A, T, P, _lib.MATH_HW, NORM, w=w, tri=cases.pack(C))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        warm = basket_price(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=td)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(warm.block.cpu().numpy(), want[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = basket_price(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=td)
    got.block.fill_(float("nan"))
    got.terminal_sum.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.block.cpu().numpy(), want[0])
    np.testing.assert_array_equal(got.terminal_sum.cpu().numpy(), want[1])
    wd.mul_(2.0)  # a replay reads the tables again
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.block.cpu().numpy(), _general(rows, A, T, P, _lib.MATH_HW, NORM, w=2.0 * w,
                                                                   tri=cases.pack(C))[0])


def test_single_path_has_zero_standard_errors() -> None:
    for A in (1, 3, 8):
        rows, w, C = _drawn(A, 6)
        tri = cases.pack(C)
        for norm in (NORM, RAW):
            for math, (eps, hw) in MATHS.items():
                ref = gr.reference(_oracle, rows, A, 3, 1, SEED, ORD0, weights=w, corr=C, normalize=bool(norm), eps=eps)
                for flags in {hw, hw | (_lib.PRICE_REPLAY if norm else 0)}:
                    got = _general(rows, A, 3, 1, flags, norm, w=w, tri=tri)
                    assert np.all(got[0][:, 6:12] == 0.0)
                    if br.exercise_count_ok(ref.doubt, 1):
                        _check(got, ref, f"single path A {A} {math} norm {norm}")
