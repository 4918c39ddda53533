"""basket_path_kernel (smc_basket_price_paths) on the device, every output into NaN-poisoned buffers: against the
independent float64 reference of tests/helpers/basket_path_reference.py in portable and SMC_MATH_HW math under both
normalisations (all 25 columns and the terminal sums within the helper's a-priori bound, which is computed, with the
condition on the flags in doubt, before the kernel's output is looked at); the bit-for-bit relations the header states
(the European columns and terminal sums are smc_basket_price_general's; without barriers the knock-out columns are the
European ones and the worst-of columns the price call's; at one date the Asian and lookback columns are the European
ones); bit-identity run to run, under a split, with the ordinal on the device, stride 0, an all-rho table and
SMC_PRICE_REPLAY; small shapes; graph capture; the Python surface; and the orderings.
tests/test_basket_path_reference.py shows on the CPU that wrong readings leave that bound."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.basket import BASKET_PATH_FIELDS, BasketConfig, BasketEngine, basket_price, basket_price_paths
from tests.helpers import assert_rows_equal, poisoned
from tests.helpers import basket_general_cases as cases
from tests.helpers import basket_path_cases as pc
from tests.helpers import basket_path_reference as pr
from tests.helpers import basket_reference as br
from tests.helpers import instantiations as inst

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED, ORD0 = pc.SEED, pc.ORD0
MATHS = {"portable": 0, "hw": _lib.MATH_HW}
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
COLS = _lib.BASKET_PATH_COLS


def _dev(a: np.ndarray | None) -> torch.Tensor | None:
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def _paths(rows: np.ndarray, A: int, T: int, P: int, flags: int, norm: int, *, w: np.ndarray | None = None,
           ws: int | None = None, tri: np.ndarray | None = None, cs: int | None = None, bars: np.ndarray | None = None,
           ordinal0: int = ORD0, ordinal_dev: torch.Tensor | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(block [B, 25], terminal sums [B, A]) of one C call; w [A] or [B, A], tri [n] or [B, n] (strides default to 0
    for a single row, to the row length otherwise), bars [B, 3]."""
    B = rows.shape[0]
    cd, wd, td, bd = _dev(rows), _dev(w), _dev(tri), _dev(bars)
    ws = (0 if w is None or w.ndim == 1 else w.shape[1]) if ws is None else ws
    cs = (0 if tri is None or tri.ndim == 1 else tri.shape[1]) if cs is None else cs
    out = poisoned((B, COLS), torch.float64, DEV)
    tsum = poisoned((B, A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price_paths(
        _lib.ptr(cd), _lib.ptr(wd), ws, _lib.ptr(td), cs, _lib.ptr(bd), B, A, T, P, SEED, _lib.ptr(ordinal_dev),
        ordinal0, flags, norm, _lib.ptr(out), _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy(), tsum.cpu().numpy()
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    return got


def _general(rows: np.ndarray, A: int, T: int, P: int, flags: int, norm: int, *, w: np.ndarray | None = None,
             tri: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    B = rows.shape[0]
    cd, wd, td = _dev(rows), _dev(w), _dev(tri)
    out = poisoned((B, _lib.BASKET_PRICE_COLS), torch.float64, DEV)
    tsum = poisoned((B, A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price_general(
        _lib.ptr(cd), _lib.ptr(wd), 0 if w is None else w.shape[1], _lib.ptr(td), 0 if tri is None else tri.shape[1], B,
        A, T, P, SEED, None, ORD0, flags, norm, _lib.ptr(out), _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tsum.cpu().numpy()


def _same(a: tuple[np.ndarray, np.ndarray], b: tuple[np.ndarray, np.ndarray], msg: str = "") -> None:
    assert_rows_equal(a[0], b[0], msg + " block")
    assert_rows_equal(a[1], b[1], msg + " terminal sums")


GROUPS = (("prices", slice(0, 10)), ("stderr", slice(10, 20)), ("means", [20, 23, 24]), ("shares", [21, 22]))


def _check(got: tuple[np.ndarray, np.ndarray], ref: pr.PathRef, label: str) -> None:
    cols, tsum = got
    used = {"sums": br.share_used(tsum, ref.tot, ref.tot_bound)}
    for name, sel in GROUPS:
        used[name] = br.share_used(cols[:, sel], ref.cols[:, sel], ref.cols_bound[:, sel])
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) <= 1.0, (label, used)  # a share is a count: it may use its whole tolerance
    assert max(v for k, v in used.items() if k != "shares") < 1.0, (label, used)


def _against_reference(case, spread: bool) -> None:
    A, T, P, B = case
    rows, w, C, bars = pc.inputs(_oracle, A, B, spread)
    tri = cases.pack(C) if A > 1 else None
    # every launch the ledger counts for the row: both maths, NORMALIZE and RAW
    for run in inst.pricing_runs_of("basket path", case):
        hw, norm = MATHS[run.math], (NORM if run.normalize else RAW)
        assert _lib.lib().smc_basket_price_paths_kernel(A, T, P, hw, norm).decode() == run.name
        ref = pc.reference(_oracle, A, T, P, B, run.math, run.normalize, spread)
        # the condition on the inputs, before the kernel's output is looked at
        assert pr.count_ok(ref.doubt[:, 0], P) and pr.count_ok(ref.doubt[:, 1], P), ref.doubt
        got = _paths(rows, A, T, P, hw, norm, w=w, tri=tri, bars=bars)
        _check(got, ref, f"paths A {A} T {T} P {P} {run.math} {'NORMALIZE' if norm else 'RAW'}")


# ---- 1. against the float64 reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=[f"A{c[0]}-T{c[1]}-P{c[2]}" for c in pc.CASES])
def test_path_kernel_columns_and_sums_against_the_reference(case) -> None:
    A, T, P, _ = case
    assert _lib.lib().smc_basket_price_paths_kernel(A, T, P, 0, NORM) == b"basket_path_kernel(replay)"
    assert _lib.lib().smc_basket_price_paths_kernel(A, T, P, _lib.MATH_HW, RAW) == b"basket_path_kernel(raw)"
    _against_reference(case, False)


def test_path_kernel_spread_against_the_reference() -> None:
    """A = 2, weights (1, -1), K = 0: levels of either sign, a lower barrier below zero."""
    rows, _, _, bars = pc.inputs(_oracle, 2, pc.SPREAD[3], True)
    assert np.any(bars[:, 0] < 0.0)
    _against_reference(pc.SPREAD, True)


# ---- 2. bit for bit against the price call -------------------------------------------------------------------------------
EUROPEAN_EXTRA = [(1, 3, 693, 6), (6, 4, 2049, 6), (7, 3, 100, 6)]


# a shape of EUROPEAN_EXTRA runs once, with its own B: the ids stay one per shape
@pytest.mark.parametrize("case", [c for c in pc.CASES if c[:3] not in [e[:3] for e in EUROPEAN_EXTRA]] + EUROPEAN_EXTRA,
                         ids=lambda c: f"A{c[0]}-T{c[1]}-P{c[2]}")
def test_european_columns_and_sums_are_the_price_call(case) -> None:
    A, T, P, B = case
    rows, w, C, bars = pc.inputs(_oracle, A, B)
    tri = cases.pack(C) if A > 1 else None
    for hw in MATHS.values():
        for norm in (NORM, RAW):
            price = _general(rows, A, T, P, hw | _lib.PRICE_REPLAY, norm, w=w, tri=tri)
            got = _paths(rows, A, T, P, hw, norm, w=w, tri=tri, bars=bars)
            assert_rows_equal(got[0][:, [8, 9, 18, 19]], price[0][:, [0, 1, 6, 7]], "European columns")
            assert_rows_equal(got[1], price[1], "terminal sums")
            # without barriers: knock-out is European, worst-of knock-out is the price call's worst-of
            free = _paths(rows, A, T, P, hw, norm, w=w, tri=tri)
            assert_rows_equal(free[0][:, [2, 3, 12, 13]], free[0][:, [8, 9, 18, 19]], "knock-out without barriers")
            assert_rows_equal(free[0][:, [6, 7, 16, 17]], price[0][:, [4, 5, 10, 11]], "worst-of without barriers")
            assert np.all(free[0][:, 21:23] == 0.0)
            # the barriers move nothing but the four knock-out columns, their errors and the two shares
            rest = [0, 1, 4, 5, 8, 9, 10, 11, 14, 15, 18, 19, 20, 23, 24]
            assert_rows_equal(free[0][:, rest], got[0][:, rest], "columns without a barrier in them")
            assert_rows_equal(free[1], got[1])


@pytest.mark.parametrize("A", [1, 3, 4, 8])
def test_one_date_makes_asian_and_lookback_european(A) -> None:
    P, B = 2049, 4
    rows, w, C, bars = pc.inputs(_oracle, A, 6)
    rows, w, bars, tri = rows[:B], w[:B], bars[:B], (cases.pack(C)[:B] if A > 1 else None)
    for hw in MATHS.values():
        for norm in (NORM, RAW):
            got = _paths(rows, A, 1, P, hw, norm, w=w, tri=tri, bars=bars)[0]
            price = _general(rows, A, 1, P, hw, norm, w=w, tri=tri)[0]
            for col in (0, 4):
                assert_rows_equal(got[:, [col, col + 1, col + 10, col + 11]], got[:, [8, 9, 18, 19]], f"column {col}")
            for col in (20, 23, 24):
                assert_rows_equal(got[:, col], price[:, 12], f"column {col}")


# ---- 3. bit-identical ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,T,P", [(4, 16, 2049), (5, 3, 1000)])
def test_run_to_run_split_ordinal_stride_table_and_replay_flag(A, T, P) -> None:
    B = 6
    rows, w, C, bars = pc.inputs(_oracle, A, B)
    tri = cases.pack(C)
    n = tri.shape[1]
    for hw in MATHS.values():
        for norm in (NORM, RAW):
            kw = dict(w=w, tri=tri, bars=bars)
            one = _paths(rows, A, T, P, hw, norm, **kw)
            _same(_paths(rows, A, T, P, hw, norm, **kw), one, "run to run")
            _same(_paths(rows, A, T, P, hw | _lib.PRICE_REPLAY, norm, **kw), one, "SMC_PRICE_REPLAY")
            parts = [_paths(rows[s], A, T, P, hw, norm, w=w[s], tri=tri[s], bars=bars[s], ordinal0=ORD0 + s.start)
                     for s in (slice(0, 3), slice(3, 6))]
            _same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), one, "3 + 3")
            od = torch.tensor([ORD0 - 2], dtype=torch.int64, device=DEV)
            _same(_paths(rows, A, T, P, hw, norm, ordinal0=2, ordinal_dev=od, **kw), one, "ordinal on the device")
            other = _paths(rows, A, T, P, hw, norm, ordinal0=ORD0 + 1, **kw)
            assert not np.array_equal(other[0][:, 0], one[0][:, 0])
            # stride 0 is the row materialised B times
            shared = _paths(rows, A, T, P, hw, norm, w=w[1], tri=tri[2], bars=bars)
            full = _paths(rows, A, T, P, hw, norm, w=np.tile(w[1], (B, 1)), tri=np.tile(tri[2], (B, 1)), bars=bars)
            _same(shared, full, "stride 0")
            assert not np.array_equal(shared[0][:, 0], one[0][:, 0])
            # an all-rho table is no table
            rho = np.repeat(rows[:, 3:4], n, axis=1)
            _same(_paths(rows, A, T, P, hw, norm, w=w, tri=rho, bars=bars), _paths(rows, A, T, P, hw, norm, w=w, bars=bars),
                  "all-rho table")


# ---- 4. small shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,T,P", [(4, 5, 1), (3, 4, 3), (4, 3, 2049), (1, 6, 693), (2, 1, 5)])
def test_small_shapes_against_the_reference(A, T, P) -> None:
    B = 6
    rows, w, C, bars = pc.inputs(_oracle, A, B)
    tri = cases.pack(C) if A > 1 else None
    for math, hw in MATHS.items():
        for norm in (NORM, RAW):
            ref = pc.reference(_oracle, A, T, P, B, math, bool(norm))
            got = _paths(rows, A, T, P, hw, norm, w=w, tri=tri, bars=bars)
            if P == 1:
                assert np.all(got[0][:, 10:20] == 0.0)
            keep = (ref.doubt <= max(2, P // 256)).all(axis=1)  # a handful of paths: a flag in doubt drops the contract
            assert keep.sum() >= B // 2
            sub = pr.PathRef(ref.tot[keep], ref.tot_bound[keep], ref.cols[keep], ref.cols_bound[keep], ref.doubt[keep],
                             ref.b[keep], ref.db[keep])
            _check((got[0][keep], got[1][keep]), sub, f"small A {A} T {T} P {P} {math} norm {norm}")


def test_empty_batch_and_rejected_scale_table() -> None:
    L = _lib.lib()
    rows, w, C, bars = pc.inputs(_oracle, 8, 6)
    out = poisoned((6, COLS), torch.float64, DEV)
    cd = _dev(rows)
    assert L.smc_basket_price_paths(_lib.ptr(cd), None, 0, None, 0, None, 0, 8, 2, 2048, SEED, None, 0, 0, NORM,
                                    _lib.ptr(out), None, None) == _lib.SMC_OK
    # 8 * 4000 scales (128000 bytes) leave no room for one date of accumulators (8 rows of 4 KiB) in 144 KiB
    assert L.smc_basket_price_paths_kernel(8, 4000, 2048, 0, NORM) == b"unsupported"
    assert L.smc_basket_price_paths(_lib.ptr(cd), None, 0, None, 0, None, 6, 8, 4000, 2048, SEED, None, 0, 0, NORM,
                                    _lib.ptr(out), None, None) == _lib.SMC_ERR_INVALID_SHAPE
    assert "scales" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---- 5. graph ------------------------------------------------------------------------------------------------------------------
def test_path_call_is_capturable_in_a_graph() -> None:
    A, T, P, B = 4, 16, 1000, 6
    rows, w, C, bars = pc.inputs(_oracle, A, B)
    tri = cases.pack(C)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=32, mc_seed=SEED, math="hw")
    cd, wd, td, bd = _dev(rows), _dev(w), _dev(tri), _dev(bars)
    want = _paths(rows, A, T, P, _lib.MATH_HW, NORM, w=w, tri=tri, bars=bars)
    kw = dict(ordinal0=ORD0, n_paths=P, weights=wd, correlation=td, barriers=bd)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        warm = basket_price_paths(cd, cfg, **kw)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert_rows_equal(warm.block.cpu().numpy(), want[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = basket_price_paths(cd, cfg, **kw)
    got.block.fill_(float("nan"))
    got.terminal_sum.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert_rows_equal(got.block.cpu().numpy(), want[0], "replayed block")
    assert_rows_equal(got.terminal_sum.cpu().numpy(), want[1], "replayed terminal sums")


# ---- 6. the Python surface -------------------------------------------------------------------------------------------------------
def test_basket_price_paths_is_the_c_call_and_knock_ins_follow_by_difference() -> None:
    A, T, P, B = 4, 5, 1000, 6
    rows, w, C, bars = pc.inputs(_oracle, A, B)
    tri = cases.pack(C)
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=64, batches_per_mc_run=32, mc_seed=SEED, math="portable")
    cd, wd, Cd, td, bd = _dev(rows), _dev(w), _dev(C), _dev(tri), _dev(bars)
    per = _paths(rows, A, T, P, 0, NORM, w=w, tri=tri, bars=bars)
    for want, kw in ((per, dict(weights=wd, correlation=Cd, barriers=bd)),
                     (per, dict(weights=wd, correlation=td, barriers=bd, validate=True)),
                     (_paths(rows, A, T, P, 0, NORM, w=w[0], tri=tri[0], bars=bars),
                      dict(weights=wd[0].contiguous(), correlation=Cd[0].contiguous(), barriers=bd)),
                     (_paths(rows, A, T, P, 0, NORM, bars=bars), dict(barriers=bd)),
                     (_paths(rows, A, T, P, 0, NORM, w=w, tri=tri), dict(weights=wd, correlation=Cd)),
                     (_paths(rows, A, T, P, 0, NORM), dict())):
        got = basket_price_paths(cd, cfg, ordinal0=ORD0, n_paths=P, **kw)
        torch.cuda.synchronize()
        assert_rows_equal(got.block.cpu().numpy(), want[0])
        assert_rows_equal(got.terminal_sum.cpu().numpy(), want[1])
        for col, name in enumerate(BASKET_PATH_FIELDS):
            np.testing.assert_array_equal(getattr(got, name).cpu().numpy(), want[0][:, col])
    with pytest.raises(ValueError, match="lower < upper"):
        basket_price_paths(cd, cfg, n_paths=P, barriers=bd[:, [1, 0, 2]].contiguous(), validate=True)
    with pytest.raises(ValueError, match="NaN"):
        basket_price_paths(cd, cfg, n_paths=P, barriers=bd * float("nan"), validate=True)
    assert basket_price_paths(cd[:0], cfg, n_paths=P, barriers=bd[:0]).block.shape == (0, COLS)
    # knock-ins by difference: European minus knock-out, the price call's worst-of minus the knocked-out worst-of
    got = basket_price_paths(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=Cd, barriers=bd)
    price = basket_price(cd, cfg, ordinal0=ORD0, n_paths=P, weights=wd, correlation=Cd)
    torch.cuda.synchronize()
    for full, err, out, oerr in ((got.european_put, got.european_put_stderr, got.knock_out_put, got.knock_out_put_stderr),
                                 (got.european_call, got.european_call_stderr, got.knock_out_call, got.knock_out_call_stderr),
                                 (price.worst_of_put, price.worst_of_put_stderr, got.worst_knock_out_put,
                                  got.worst_knock_out_put_stderr),
                                 (price.worst_of_call, price.worst_of_call_stderr, got.worst_knock_out_call,
                                  got.worst_knock_out_call_stderr)):
        assert bool(((full - out) >= -(err + oerr)).all())
    assert bool((got.knocked_share > 0).any()) and bool((got.worst_knocked_share > 0).any())


def test_engine_price_paths_is_the_c_call() -> None:
    A, T, N, M, B = 3, 4, 64, 32, 6
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="hw")
    eng = BasketEngine(cfg, B, device=torch.device(DEV))
    eng.set_position(0, 0)
    eng.enqueue_step()
    _, w, C, _ = pc.inputs(_oracle, A, B)
    torch.cuda.synchronize()
    rows = eng.buffers.contracts.cpu().numpy()
    bars = pr.default_barriers(rows, A, w, C)
    got = eng.price_paths(ordinal0=ORD0, n_paths=693, weights=_dev(w), correlation=_dev(C), barriers=_dev(bars))
    torch.cuda.synchronize()
    want = _paths(rows, A, T, 693, _lib.MATH_HW, NORM, w=w, tri=cases.pack(C), bars=bars)
    assert_rows_equal(got.block.cpu().numpy(), want[0])
    assert_rows_equal(got.terminal_sum.cpu().numpy(), want[1])


# ---- 7. orderings ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES + [pc.SPREAD], ids=lambda c: f"A{c[0]}-T{c[1]}-P{c[2]}")
def test_orderings(case) -> None:
    """Per path the knock-out payoff is the European one or 0, mnb <= b_last <= mxb and payoffs are monotone, and each
    pair of sums runs over the same paths in the same order: the first four hold exactly."""
    A, T, P, B = case
    rows, w, C, bars = pc.inputs(_oracle, A, B, case == pc.SPREAD)
    for hw in MATHS.values():
        for norm in (NORM, RAW):
            c = _paths(rows, A, T, P, hw, norm, w=w, tri=cases.pack(C) if A > 1 else None, bars=bars)[0]
            assert np.all(c[:, 2] <= c[:, 8]) and np.all(c[:, 3] <= c[:, 9])
            assert np.all(c[:, 4] >= c[:, 8]) and np.all(c[:, 5] >= c[:, 9])
            assert np.all(c[:, 24] <= c[:, 20]) and np.all(c[:, 20] <= c[:, 23])
            assert np.all(c[:, :20] >= 0.0) and np.all(c[:, 21:23] >= 0.0) and np.all(c[:, 21:23] <= 1.0)
