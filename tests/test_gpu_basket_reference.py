"""The four basket kernels of csrc/basket.hip (basket_kernel, basket_cf_kernel, basket_resident_kernel,
basket_price_kernel) against the independent float64 reference of tests/helpers/basket_reference.py, in portable and
in SMC_MATH_HW math: every stored path element, terminal sum, target and price column within the a-priori bound the
helper derives from the reference's own values (computed before the kernel's output is looked at), into NaN-poisoned
buffers.  tests/test_gpu_basket.py and tests/test_gpu_basket_price.py show the kernels equal to the oracle's
restatement bit for bit; that restatement was written from the kernels, so this file is what says both are right.
tests/test_basket_reference.py holds the oracle's kernel mode to the same reference on the CPU, and shows that wrong
readings of the engine leave the bounds.

The dynamic tail and the multi-round schedules of basket_resident_kernel stay with the bit-exact tests: a float64
reference adds nothing to an order of summation, and their shapes are too large for it.  The B = 70 case runs more
contracts than one coefficient table holds (64); a launch has floor(#CUs / W) contract sequences, though, so every
sequence still takes one contract there.  A second table fill needs more than 64 static contracts in one sequence:
test_resident_kernel_second_coefficient_table_fill gets there with a launch on a stream masked to one CU."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.basket import BasketConfig, BasketEngine, basket_price, basket_targets
from tests.helpers import basket_reference as br
from tests.helpers import instantiations as inst
from tests.helpers import poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7
ORD0 = 3
MATHS = {"portable": br.PORTABLE, "hw": br.HW}


def _sobol_rows(A: int, n: int, skip: int = 0) -> np.ndarray:
    _oracle.build()
    lo, hi = BasketConfig(n_assets=A, network_size=64, batches_per_mc_run=32).arrays()
    return _oracle.sobol_contracts(SEED, skip, n, lo, hi)


def _reference(rows: np.ndarray, A: int, T: int, P: int, math: str, **kw) -> br.BasketRef:
    ref = br.reference(_oracle, rows, A, T, P, SEED, kw.pop("ordinal0", ORD0), eps=MATHS[math], **kw)
    assert br.exercise_count_ok(ref.doubt, P), ref.doubt
    return ref


def _train(rows: np.ndarray, A: int, T: int, N: int, M: int, math: str, *, resident: bool, store: bool,
           pitch: int = 0, keep_sums: bool = True) -> tuple[np.ndarray | None, np.ndarray | None, np.ndarray]:
    """(stored paths [B, A, T, pitch or P] or None, terminal sums or None, targets) of one training call.
    keep_sums = False passes no terminal-sum buffer: the split pair's kernel then runs fused (basket_kernel<A, HW, 0>)."""
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math=math)
    B = rows.shape[0]
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    paths = poisoned((B, A, T, pitch or N * M), torch.float32, DEV) if store else None
    tsum = poisoned((B, A), torch.float64, DEV) if keep_sums else None
    tg = poisoned((B, N), torch.complex64, DEV)
    basket_targets(cd, cfg, ordinal0=ORD0, paths=paths, terminal_sum=tsum, targets=tg, pitch=pitch, resident=resident)
    torch.cuda.synchronize()
    return (paths.cpu().numpy() if store else None), (tsum.cpu().numpy() if keep_sums else None), tg.cpu().numpy()


def _check_training(got: tuple, ref: br.BasketRef, label: str) -> None:
    paths, tsum, tg = got
    P = ref.xT.shape[-1]
    used = {"targets": br.complex_share_used(tg, ref.targets, ref.targets_bound)}
    if tsum is not None:
        assert not np.isnan(tsum).any(), label
        used["sums"] = br.share_used(tsum, ref.tot, ref.tot_bound)
    if paths is not None:
        assert not np.isnan(paths[..., :P]).any(), label
        assert np.isnan(paths[..., P:]).all(), f"{label}: the padding of the pitch was written"
        used["paths"] = br.share_used(paths[..., :P], ref.x, ref.paths_bound)
    assert not np.isnan(tg).any(), label
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) < 1.0, (label, used)


def _name(A: int, T: int, N: int, M: int, resident: bool) -> str:
    return _lib.lib().smc_basket_train_targets_kernel(A, T, N, M, 1 if resident else 0, 1).decode()


# ---- basket_kernel + basket_cf_kernel --------------------------------------------------------------------------------
# (A, T, N, M, padded pitch): basket_kernel<A, HW, MODE> is instantiated per asset count with unrolled Cholesky and
# driver code, so every A = 1 .. 8 runs, in both math modes, split (MODE 1 + basket_cf_kernel: the terminal sums kept)
# and fused (MODE 0); tests/test_instantiation_ledger.py holds this table to the ledger of instantiations
SPLIT_CASES = [(1, 5, 64, 32, False), (2, 16, 64, 32, False), (3, 16, 64, 32, True), (5, 1, 64, 32, False),
               (7, 3, 64, 32, False), (8, 5, 64, 32, False), (4, 16, 64, 64, False),
               (1, 3, 64, 32, False), (2, 3, 64, 32, False), (3, 3, 64, 32, False), (4, 3, 64, 32, False),
               (5, 3, 64, 32, False), (6, 3, 64, 32, False), (8, 3, 64, 32, False)]


@pytest.mark.parametrize("A,T,N,M,padded", SPLIT_CASES)
def test_split_pair_stored_paths_sums_and_targets(A, T, N, M, padded) -> None:
    assert _name(A, T, N, M, False) == "basket_kernel+basket_cf_kernel"
    assert _lib.lib().smc_basket_train_targets_kernel(A, T, N, M, 0, 0) == b"basket_kernel"  # no sums kept: fused
    rows = _sobol_rows(A, 6)
    pitch = int(_lib.lib().smc_path_pitch(N * M, 0)) if padded else 0
    assert not padded or pitch > N * M
    for math in MATHS:
        ref = _reference(rows, A, T, N * M, math, N=N, M=M, keep_paths=True)
        got = _train(rows, A, T, N, M, math, resident=False, store=True, pitch=pitch)
        _check_training(got, ref, f"split pair A {A} T {T} P {N * M} {math}")
        got = _train(rows, A, T, N, M, math, resident=False, store=True, pitch=pitch, keep_sums=False)
        _check_training(got, ref, f"fused A {A} T {T} P {N * M} {math}")


# ---- basket_resident_kernel ------------------------------------------------------------------------------------------
# (A, N, M, W): every asset count the resident kernel's LDS budget admits (A <= 6) at one workgroup per contract
RESIDENT_CASES = [(4, 256, 16, 1), (6, 256, 32, 2), (3, 2048, 6, 3),
                  (1, 256, 16, 1), (2, 256, 16, 1), (3, 256, 16, 1), (5, 256, 16, 1), (6, 256, 16, 1)]


@pytest.mark.parametrize("A,N,M,W", RESIDENT_CASES)
def test_resident_kernel_stored_and_terminal_only(A, N, M, W) -> None:
    T, B = 16, 4
    assert _name(A, T, N, M, True) == "basket_resident_kernel" and N * M == W * 4096
    rows = _sobol_rows(A, B, skip=3)
    for math in MATHS:
        ref = _reference(rows, A, T, N * M, math, N=N, M=M, keep_paths=True)
        for store in (True, False):
            got = _train(rows, A, T, N, M, math, resident=True, store=store)
            _check_training(got, ref, f"resident W {W} A {A} {math} {'stored' if store else 'terminal only'}")


def test_resident_kernel_more_contracts_than_one_coefficient_table() -> None:
    A, T, N, M, B = 2, 16, 64, 64, 70
    assert _name(A, T, N, M, True) == "basket_resident_kernel"
    rows = _sobol_rows(A, B, skip=11)
    for math in MATHS:
        ref = _reference(rows, A, T, N * M, math, N=N, M=M)
        got = _train(rows, A, T, N, M, math, resident=True, store=False)
        _check_training(got, ref, f"resident B {B} {math}")


def test_resident_kernel_second_coefficient_table_fill() -> None:
    """More than 64 contracts in ONE contract sequence: the launch goes to a stream masked to a single CU, so it has
    one sequence (W = 1) of B = 96 contracts, of which the first 72 are static (wave 0 fills the coefficient table at
    iterations 0 and 64) and the last 24 come from the dynamic queue.  The sync area passed is the size of a
    one-sequence launch (basket.hip basket_sync_layout: 128 + 128 groups, the slice sums, rounded up to 256, the
    column sums), which a launch of two or more sequences rejects: so the mask was honoured."""
    from spectralmc_amd.gbm_trainer import _destroy_streams, _masked_stream  # noqa: PLC0415

    A, T, N, M, B = 2, 16, 64, 64, 96
    assert _name(A, T, N, M, True) == "basket_resident_kernel"
    rows = _sobol_rows(A, B, skip=11)
    nsync = (128 + 128 + 4 * (A + 1) * 8 + 255) // 256 * 256 + B * N * 8
    dev = torch.device("cuda:0")
    words = (torch.cuda.get_device_properties(dev).multi_processor_count + 31) // 32
    owned: list[int] = []
    one_cu = _masked_stream(dev, [1] + [0] * (words - 1), owned)
    try:
        for math in MATHS:
            ref = _reference(rows, A, T, N * M, math, N=N, M=M)
            cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
            scratch = torch.empty((B, A, N * M), dtype=torch.float32, device=DEV)
            tsum = poisoned((B, A), torch.float64, DEV)
            tg = poisoned((B, N), torch.complex64, DEV)
            sync = torch.zeros(nsync, dtype=torch.uint8, device=DEV)
            torch.cuda.synchronize()
            _lib.check(_lib.lib().smc_basket_train_targets(
                _lib.ptr(cd), B, A, T, N, M, SEED, None, ORD0, _lib.MATH_HW if math == "hw" else 0, 1,
                _lib.STORE_TERMINAL, _lib.ptr(scratch), N * M, B, _lib.ptr(tsum), _lib.ptr(tg), _lib.ptr(sync), nsync,
                _lib.stream_handle(one_cu)))
            torch.cuda.synchronize()
            _check_training((None, tsum.cpu().numpy(), tg.cpu().numpy()), ref, f"resident, one sequence of {B}, {math}")
    finally:
        torch.cuda.synchronize()
        _destroy_streams(owned)


# ---- basket_price_kernel ---------------------------------------------------------------------------------------------
def _price(rows: np.ndarray, A: int, T: int, P: int, flags: int, norm: int,
           ordinal0: int = ORD0) -> tuple[np.ndarray, np.ndarray]:
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    out = poisoned((rows.shape[0], _lib.BASKET_PRICE_COLS), torch.float64, DEV)
    tsum = poisoned((rows.shape[0], A), torch.float64, DEV)
    _lib.check(_lib.lib().smc_basket_price(_lib.ptr(cd), rows.shape[0], A, T, P, SEED, None, ordinal0, flags, norm,
                                           _lib.ptr(out), _lib.ptr(tsum), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tsum.cpu().numpy()


def _check_price(got: tuple[np.ndarray, np.ndarray], ref: br.BasketRef, label: str) -> None:
    cols, tsum = got
    P = ref.xT.shape[-1]
    assert not np.isnan(cols).any() and not np.isnan(tsum).any(), label
    used = {"sums": br.share_used(tsum, ref.tot, ref.tot_bound)}
    for name, sel in (("prices", slice(0, 6)), ("stderr", slice(6, 12)), ("means", slice(12, 15)),
                      ("exercise", slice(15, 16)), ("intrinsic", slice(16, 18))):
        used[name] = br.share_used(cols[:, sel], ref.cols[:, sel], ref.cols_bound[:, sel])
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) <= 1.0, (label, used)  # the exercise share is a count: it may use its whole tolerance
    assert max(v for k, v in used.items() if k != "exercise") < 1.0, (label, used)
    if P == 1:
        assert np.all(cols[:, 6:12] == 0.0), label


def _price_against_reference(rows: np.ndarray, A: int, T: int, P: int, label: str) -> None:
    """Every launch the ledger counts for the row (both maths, raw, lds and forced replay), each under the name the
    library's own query gives it."""
    name = _lib.lib().smc_basket_price_kernel
    refs = {}
    for run in inst.pricing_runs_of("basket price", (A, T, P, rows.shape[0])):
        flags = (_lib.MATH_HW if run.math == "hw" else 0) | (_lib.PRICE_REPLAY if run.force_replay else 0)
        norm = _lib.NORM_NORMALIZE if run.normalize else _lib.NORM_RAW
        assert name(A, T, P, flags, norm).decode() == run.name
        if (run.math, run.normalize) not in refs:
            refs[run.math, run.normalize] = _reference(rows, A, T, P, run.math, normalize=run.normalize)
        _check_price(_price(rows, A, T, P, flags, norm), refs[run.math, run.normalize], f"{label} {run.math} {run.name}")


# (A, T, P, B): a single path, a ragged chunk, one path into the second chunk and two full chunks at A = 1, 3, 4, 8;
# then the asset counts those leave out, at the ledger's shape (one stream per group, a ragged lane, a partial chunk).
# tests/test_instantiation_ledger.py holds this table to the ledger of instantiations
PRICE_CASES = [(A, T, P, 6) for A, T in [(1, 3), (3, 5), (4, 16), (8, 2)] for P in [1, 693, 2049, 4096]]
LEDGER_PRICE_CASES = [(2, 3, 693, 3), (5, 3, 693, 3), (6, 3, 693, 3), (7, 3, 693, 3)]
PRICE_CASES += LEDGER_PRICE_CASES


@pytest.mark.parametrize("P", [1, 693, 2049, 4096])
@pytest.mark.parametrize("A,T", [(1, 3), (3, 5), (4, 16), (8, 2)])
def test_price_kernel_columns_and_sums(A, T, P) -> None:
    """A single path, a ragged chunk, one path into the second chunk, two full chunks."""
    assert (A, T, P, 6) in PRICE_CASES
    _price_against_reference(_sobol_rows(A, 6), A, T, P, f"price A {A} T {T} P {P}")


@pytest.mark.parametrize("A,T,P,B", LEDGER_PRICE_CASES)
def test_price_kernel_columns_and_sums_at_every_asset_count(A, T, P, B) -> None:
    _price_against_reference(_sobol_rows(A, B), A, T, P, f"price A {A} T {T} P {P}")


# ---- the hand-built rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,T,M", [(2, 16, 32), (4, 5, 64), (8, 3, 32)])
def test_hand_built_rows_through_both_calls(A, T, M) -> None:
    N = 64
    hand = br.hand_built_rows(A)
    rows = np.stack(list(hand.values()))
    assert rows.shape[0] <= 6 and ("rho 1" in hand) == (A == 2)
    for math in MATHS:
        ref = _reference(rows, A, T, N * M, math, N=N, M=M, keep_paths=True)
        got = _train(rows, A, T, N, M, math, resident=False, store=True)
        _check_training(got, ref, f"hand-built A {A} {math}")
    _price_against_reference(rows, A, T, N * M, f"hand-built price A {A}")
    _price_against_reference(rows, A, T, 693, f"hand-built price A {A} P 693")


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_engine_and_basket_price_give_the_reference_columns() -> None:
    A, T, N, M, B = 3, 8, 64, 32, 6
    cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="portable")
    eng = BasketEngine(cfg, B, device=torch.device(DEV))
    eng.set_position(0, 0)
    eng.enqueue_step()
    got = eng.price()
    torch.cuda.synchronize()
    rows = eng.buffers.contracts.cpu().numpy()  # the contracts the engine reports
    assert rows.shape == (B, cfg.dim) and not np.isnan(rows).any()
    ref = _reference(rows, A, T, N * M, "portable", N=N, M=M, ordinal0=0)
    _check_price((got.block.cpu().numpy(), got.terminal_sum.cpu().numpy()), ref, "BasketEngine.price")
    _check_training((None, eng.terminal_sum.cpu().numpy(), eng.buffers.targets.cpu().numpy()), ref, "BasketEngine step")
    odd = basket_price(eng.buffers.contracts, cfg, ordinal0=2, n_paths=693)
    torch.cuda.synchronize()
    _check_price((odd.block.cpu().numpy(), odd.terminal_sum.cpu().numpy()),
                 _reference(rows, A, T, 693, "portable", ordinal0=2), "basket_price, 693 paths at ordinal 2")
    hw_cfg = BasketConfig(n_assets=A, timesteps=T, network_size=N, batches_per_mc_run=M, mc_seed=SEED, math="hw",
                          normalize=False)
    hw = basket_price(eng.buffers.contracts, hw_cfg, ordinal0=ORD0)
    torch.cuda.synchronize()
    _check_price((hw.block.cpu().numpy(), hw.terminal_sum.cpu().numpy()),
                 _reference(rows, A, T, N * M, "hw", normalize=False), "basket_price, hw math, RAW")
