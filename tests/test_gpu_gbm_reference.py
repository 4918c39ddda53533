"""The single-asset kernels of csrc/gbm.hip against the independent float64 reference of
tests/helpers/gbm_reference.py, in portable and in SMC_MATH_HW math: every stored path element, row sum, target bin and
price column within the a-priori bound the helper derives from the reference's own values (computed before the
kernel's output is looked at), into NaN-poisoned buffers, no element excluded.  SMC_MATH_HW cannot be restated on a
CPU (hw_log_increments4, hw_log_pair, hw_log_tail4, advance_packed and the HW instantiations of every kernel have code
of their own): this file is what holds it per element.  In portable math the kernels are bit-exact with the oracle's
kernel mode (tests/test_gpu_engine.py), which tests/test_gbm_reference.py holds to the same reference on the CPU; the
portable cases here assert that the stored paths use exactly the share of the bound the oracle's kernel mode uses,
which ties the two files.

Each case asserts the name of the kernel it means to reach, and TRAIN_CASES holds a row for every template
instantiation of the training kernels that launch_engine<float> can select (tests/helpers/instantiations.py, held to
the dispatch's text and to this table by tests/test_instantiation_ledger.py).  The contracts are those of the CPU sweep
(tests/test_gbm_reference.case_rows: Sobol-drawn rows in the default bounds and the hand-built ones)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from spectralmc_amd.sobol_sampler import SobolEngine
from tests.helpers import gbm_reference as gref
from tests.helpers import instantiations as inst
from tests.helpers import make_domain_bounds, poisoned
from tests.test_gbm_reference import REST, SEED, case_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
ORD0 = 3
MATHS = {"portable": (gref.PORTABLE, 0), "hw": (gref.HW, _lib.MATH_HW)}


@functools.lru_cache(maxsize=8)
def _ref(B: int, T: int, P: int, scheme: int, normalize: bool, math: str, N: int = 0, M: int = 0, bars: bool = False,
         keep_paths: bool = False, ordinal0: int = ORD0) -> gref.GbmRef:
    """The reference of the first B case rows, once per shape."""
    _oracle.build()
    rows, barriers = case_rows(scheme, normalize)
    ref = gref.reference(_oracle, rows[:B], T, P, SEED, ordinal0, scheme=scheme, eps=MATHS[math][0], N=N, M=M,
                         normalize=normalize, bars=barriers[:B] if bars else None, keep_paths=keep_paths)
    if bars:  # the count condition, on the reference alone
        assert gref.count_ok(ref.doubt, P), ref.doubt
    return ref


# ---- the training kernels ----------------------------------------------------------------------------------------------
def _train_targets(rows: np.ndarray, T: int, N: int, M: int, scheme: int, normalize: bool, flags: int, store: int,
                   pitch: int, *, ordinal0: int = ORD0, ordinal_dev: torch.Tensor | None = None,
                   with_rowsum: bool = False, sliced: bool = False) -> tuple[np.ndarray, np.ndarray | None, np.ndarray]:
    """(stored rows [B, T, P] or terminal rows [B, P], row sums [B, T] or None, targets [B, N]) of one smc_train_targets."""
    L = _lib.lib()
    B, P = rows.shape[0], N * M
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    paths = poisoned((B, T, pitch) if store == _lib.STORE_ALL else (B, pitch), torch.float32, DEV)
    rowsum = poisoned((B, T), torch.float64, DEV) if with_rowsum else None
    tg = poisoned((B, N), torch.complex64, DEV)
    wsb = int(L.smc_engine_workspace_bytes(B, T, P, int(with_rowsum))) if sliced else 0
    assert not sliced or wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV) if sliced else None
    _lib.check(L.smc_train_targets(_lib.ptr(cd), B, T, N, M, SEED, _lib.ptr(ordinal_dev), ordinal0, scheme | flags,
                                   int(normalize), _lib.DTYPE_F32, store, _lib.ptr(paths), pitch, B, _lib.ptr(rowsum),
                                   _lib.ptr(tg), _lib.ptr(ws), wsb, None))
    torch.cuda.synchronize()
    return paths[..., :P].cpu().numpy(), (rowsum.cpu().numpy() if with_rowsum else None), tg.cpu().numpy()


def _check_training(got: tuple, ref: gref.GbmRef, store: int, label: str) -> dict[str, float]:
    paths, rowsum, tg = got
    assert not np.isnan(paths).any() and not np.isnan(tg).any(), label
    want, bound = (ref.x, ref.dx) if store == _lib.STORE_ALL else (ref.xT, ref.dxT)
    used = {"paths": gref.share_used(paths, want, bound),
            "targets": gref.complex_share_used(tg, ref.targets, ref.targets_bound)}
    if rowsum is not None:
        assert not np.isnan(rowsum).any(), label
        used["row sums"] = gref.share_used(rowsum, ref.rowsum, ref.rowsum_bound)
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) < 1.0, (label, used)
    return used


def _kernel_mode_paths_share(B: int, T: int, P: int, scheme: int, ref: gref.GbmRef, store: int, ordinal0: int = ORD0) -> float:
    """The share of the path bound the oracle's kernel mode uses: what the CPU sweep measures."""
    rows, _ = case_rows(scheme, True)
    kp, term, _ = _oracle.kernel_paths(rows[:B], T, P, SEED, ordinal0, scheme, want_paths=True)
    return gref.share_used(kp, ref.x, ref.dx) if store == _lib.STORE_ALL else gref.share_used(term, ref.xT, ref.dxT)


ALL, TERMINAL, LOG, SIMPLE = _lib.STORE_ALL, _lib.STORE_TERMINAL, gref.LOG_EULER, gref.SIMPLE_EULER
# (kernel, B, T, N, M, scheme, normalize, store, padded pitch, sliced).  tests/test_instantiation_ledger.py holds this
# table, by the host rules of csrc/gbm.hip, to the ledger of instantiations launch_engine<float> can select: the rows
# below "one row per instantiation" are the smallest shapes that select each one the rows above do not reach.
TRAIN_CASES = [
    ("resident_kernel", 12, 16, 64, 64, LOG, True, ALL, True, False),            # straight-line 16-row block
    ("resident_kernel", 12, 16, 64, 64, SIMPLE, True, ALL, True, False),         # ... its simple-Euler instantiation
    ("resident_kernel", 12, 5, 64, 64, LOG, True, ALL, True, False),             # rolled rows, odd T: the tail
    ("resident_kernel", 12, 20, 64, 64, LOG, True, ALL, True, False),            # rolled rows, T > 16
    ("resident_kernel", 3, 16, 512, 96, LOG, True, ALL, True, False),            # 12 chunks: registers beyond LDS
    ("packed_kernel", 12, 16, 64, 8, LOG, True, ALL, True, False),               # P = 512
    ("packed_kernel", 12, 5, 64, 32, LOG, False, ALL, True, False),              # P = 2048, odd T, RAW
    ("packed_kernel", 12, 5, 64, 32, SIMPLE, True, ALL, True, False),            # ... in simple Euler
    ("packed_kernel", 12, 1, 16, 64, LOG, True, ALL, True, False),               # P = 1024, T = 1: the stream span
    ("wave_kernel", 12, 1, 16, 64, LOG, False, ALL, True, False),                # T = 1, N = 16, P = 1024
    ("wave_kernel", 12, 2, 64, 64, LOG, False, ALL, True, False),                # T = 2, N = 64, P = 4096
    ("wave_kernel", 12, 2, 64, 64, SIMPLE, False, ALL, True, False),             # ... in simple Euler
    ("paths_kernel+cf_kernel", 12, 16, 1000, 4, LOG, True, ALL, True, False),    # the split pair, P = 4000: not straight
    ("rows_kernel+cf_kernel", 12, 17, 2048, 2, LOG, True, ALL, True, False),     # odd T beyond one row block, N > 1024
    ("rows_kernel+cf_kernel", 12, 3, 64, 96, LOG, True, ALL, True, False),       # P = 6144
    ("contract_kernel", 12, 7, 99, 7, SIMPLE, True, ALL, False, False),          # ragged P = 693
    ("contract_kernel", 12, 20, 100, 30, SIMPLE, True, ALL, False, False),       # P = 3000, row-block replay
    ("contract_kernel", 12, 7, 99, 7, LOG, True, ALL, False, False),             # ... the odd tail in log-Euler
    ("queue_kernel", 12, 4, 99, 101, LOG, True, ALL, False, True),               # sliced contracts: P = 9999 > 8192
    # ---- one row per instantiation ----
    # resident_kernel<.., T16>, <.., rolled> and <.., ONTHEFLY> (RAW, whole contracts, T != 16; T >= 3, or RAW goes
    # to wave_kernel) at P = 4096
    ("resident_kernel", 12, 16, 64, 64, LOG, True, TERMINAL, True, False),
    ("resident_kernel", 12, 16, 64, 64, SIMPLE, True, TERMINAL, True, False),
    ("resident_kernel", 12, 5, 64, 64, LOG, True, TERMINAL, True, False),
    ("resident_kernel", 12, 5, 64, 64, SIMPLE, True, ALL, True, False),
    ("resident_kernel", 12, 5, 64, 64, SIMPLE, True, TERMINAL, True, False),
    ("resident_kernel", 12, 5, 64, 64, LOG, False, ALL, True, False),
    ("resident_kernel", 12, 5, 64, 64, LOG, False, TERMINAL, True, False),
    ("resident_kernel", 12, 5, 64, 64, SIMPLE, False, ALL, True, False),
    ("resident_kernel", 12, 5, 64, 64, SIMPLE, False, TERMINAL, True, False),
    # packed_kernel<.., T16> and <.., rolled> at P = 512 (eight contracts per workgroup), RAW on the T16 simple rows
    ("packed_kernel", 12, 16, 64, 8, LOG, True, TERMINAL, True, False),
    ("packed_kernel", 12, 16, 64, 8, SIMPLE, False, ALL, True, False),
    ("packed_kernel", 12, 16, 64, 8, SIMPLE, False, TERMINAL, True, False),
    ("packed_kernel", 12, 5, 64, 8, LOG, True, TERMINAL, True, False),
    ("packed_kernel", 12, 5, 64, 8, SIMPLE, True, TERMINAL, True, False),
    # wave_kernel<.., 1> and <.., 2> at P = 1024
    ("wave_kernel", 12, 1, 16, 64, LOG, False, TERMINAL, True, False),
    ("wave_kernel", 12, 1, 16, 64, SIMPLE, False, ALL, True, False),
    ("wave_kernel", 12, 1, 16, 64, SIMPLE, False, TERMINAL, True, False),
    ("wave_kernel", 12, 2, 16, 64, LOG, False, TERMINAL, True, False),
    ("wave_kernel", 12, 2, 16, 64, SIMPLE, False, TERMINAL, True, False),
    # the straight paths_kernel: T = 16 and whole 2048-path chunks in a shape neither resident_kernel (P not a
    # multiple of 4096) nor packed_kernel (P > 2048) takes: three chunks
    ("paths_kernel+cf_kernel", 12, 16, 64, 96, LOG, True, ALL, True, False),
    ("paths_kernel+cf_kernel", 12, 16, 64, 96, LOG, True, TERMINAL, True, False),
    ("paths_kernel+cf_kernel", 12, 16, 64, 96, SIMPLE, True, ALL, True, False),
    ("paths_kernel+cf_kernel", 12, 16, 64, 96, SIMPLE, True, TERMINAL, True, False),
    # the other paths_kernel (one instantiation for either store mode) at an odd P: one padding element before the
    # 8-byte-aligned terminal sum
    ("paths_kernel+cf_kernel", 12, 7, 99, 7, LOG, True, ALL, True, False),
    ("paths_kernel+cf_kernel", 12, 7, 99, 7, SIMPLE, True, ALL, True, False),
    ("paths_kernel+cf_kernel", 12, 7, 99, 7, SIMPLE, True, TERMINAL, True, False),
    # rows_kernel<float>
    ("rows_kernel+cf_kernel", 12, 3, 64, 96, LOG, True, TERMINAL, True, False),
    ("rows_kernel+cf_kernel", 12, 3, 64, 96, SIMPLE, True, ALL, True, False),
    ("rows_kernel+cf_kernel", 12, 3, 64, 96, SIMPLE, True, TERMINAL, True, False),
    ("rows_kernel+cf_kernel", 12, 17, 2048, 2, SIMPLE, True, TERMINAL, True, False),
    # queue_kernel<float> in simple Euler, without and with row sums
    ("queue_kernel", 12, 4, 99, 101, SIMPLE, True, ALL, False, True),
]


def _case_id(case: tuple) -> str:
    """The columns but the store mode, which only the terminal-row cases name."""
    return "-".join(str(v) for v in case[:7] + case[8:]) + ("-terminal" if case[7] == TERMINAL else "")


@pytest.mark.parametrize("kernel,B,T,N,M,scheme,normalize,store,padded,sliced", TRAIN_CASES,
                         ids=[_case_id(c) for c in TRAIN_CASES])
def test_train_targets_paths_sums_and_targets(kernel, B, T, N, M, scheme, normalize, store, padded, sliced) -> None:
    L = _lib.lib()
    P = N * M
    pitch = int(L.smc_path_pitch(P, 0)) if padded else P
    query = _lib.DTYPE_F32 | (0 if normalize else _lib.QUERY_RAW)
    assert L.smc_train_targets_kernel(T, N, P, query, pitch, int(sliced)).decode() == kernel
    rows, _ = case_rows(scheme, normalize)
    for math, (_, flags) in MATHS.items():
        ref = _ref(B, T, P, scheme, normalize, math, N, M, keep_paths=True)
        label = (f"{kernel} T {T} N {N} M {M} {'log' if scheme == LOG else 'simple'} {'NORM' if normalize else 'RAW'} "
                 f"{'ALL' if store == ALL else 'TERMINAL'} {math}")
        got = _train_targets(rows[:B], T, N, M, scheme, normalize, flags, store, pitch, sliced=sliced)
        used = _check_training(got, ref, store, label)
        if math == "portable":
            assert used["paths"] == _kernel_mode_paths_share(B, T, P, scheme, ref, store), label
        if kernel in ("contract_kernel", "queue_kernel"):  # these also hand out every row's sum
            got = _train_targets(rows[:B], T, N, M, scheme, normalize, flags, store, pitch, sliced=sliced, with_rowsum=True)
            _check_training(got, ref, store, label + " with row sums")


def test_sliced_resident_kernel_terminal_rows_and_targets() -> None:
    """smc_train_step at P = 131,072: two co-resident resident_kernel workgroups per contract, STORE_TERMINAL.  The
    contracts are the step's own Sobol draw (checked against the host engine), the reference is taken on them."""
    L = _lib.lib()
    B, T, N, M = 4, 16, 128, 1024
    P = N * M
    pitch = int(L.smc_path_pitch(P, 0))
    assert L.smc_train_step_kernel(T, N, M, _lib.DTYPE_F32, pitch) == b"resident_kernel(sliced)"
    lo, hi = make_domain_bounds().arrays()
    eng = SobolEngine(6, SEED, 0)
    tables = torch.from_numpy(eng.tables().view(np.int32)).to(DEV)
    lod, hid = torch.from_numpy(lo).to(DEV), torch.from_numpy(hi).to(DEV)
    nsync = int(L.smc_train_step_sync_bytes(T, N, M, _lib.DTYPE_F32, pitch))
    assert nsync > 4
    sync = torch.zeros(nsync, dtype=torch.uint8, device=DEV)
    start = [40, 9]
    _oracle.build()
    want_rows = _oracle.sobol_contracts(SEED, start[0], B, lo, hi)
    refs = {}
    for math, (eps, flags) in MATHS.items():
        cur = torch.tensor(start, dtype=torch.int64, device=DEV)
        c = poisoned((B, 6), torch.float64, DEV)
        f = poisoned((B, 6), torch.float32, DEV)
        paths = poisoned((B, pitch), torch.float32, DEV)
        tg = poisoned((B, N), torch.complex64, DEV)
        _lib.check(L.smc_train_step(_lib.ptr(tables), 6, _lib.ptr(lod), _lib.ptr(hid), _lib.ptr(cur), 0, B, _lib.ptr(c),
                                    _lib.ptr(f), B, T, N, M, SEED, _lib.SCHEME_LOG_EULER | flags, _lib.NORM_NORMALIZE,
                                    _lib.DTYPE_F32, _lib.STORE_TERMINAL, _lib.ptr(paths), pitch, B, _lib.ptr(tg),
                                    _lib.ptr(sync), nsync, None))
        torch.cuda.synchronize()
        assert cur.tolist() == [start[0] + B, start[1] + B]
        np.testing.assert_array_equal(c.cpu().numpy(), want_rows)
        if math not in refs:
            refs[math] = gref.reference(_oracle, want_rows, T, P, SEED, start[1], eps=eps, N=N, M=M)
        _check_training((paths[:, :P].cpu().numpy(), None, tg.cpu().numpy()), refs[math], _lib.STORE_TERMINAL,
                        f"resident_kernel(sliced) W 2 {math}")


# ---- ordinals --------------------------------------------------------------------------------------------------------
def test_ordinals_beyond_32_bits_and_on_the_device() -> None:
    """ordinal0 above 2^32 (the streams are keyed by ordinal_lo and ordinal_hi), given whole and split between the
    argument and the device word."""
    L = _lib.lib()
    B, T, N, M = 12, 5, 64, 64
    P, far = N * M, (1 << 32) + 12345
    pitch = int(L.smc_path_pitch(P, 0))
    assert L.smc_train_targets_kernel(T, N, P, _lib.DTYPE_F32, pitch, 0) == b"resident_kernel"
    rows, _ = case_rows(LOG, True)
    near = _ref(B, T, P, LOG, True, "portable", N, M, keep_paths=True, ordinal0=12345)
    for math, (_, flags) in MATHS.items():
        ref = _ref(B, T, P, LOG, True, math, N, M, keep_paths=True, ordinal0=far)
        assert not np.array_equal(ref.xT, near.xT)  # ordinal_hi reaches the stream
        got = _train_targets(rows[:B], T, N, M, LOG, True, flags, ALL, pitch, ordinal0=far)
        _check_training(got, ref, ALL, f"ordinal0 2^32 + 12345 {math}")
        od = torch.tensor([1 << 32], dtype=torch.int64, device=DEV)
        got = _train_targets(rows[:B], T, N, M, LOG, True, flags, ALL, pitch, ordinal0=12345, ordinal_dev=od)
        _check_training(got, ref, ALL, f"ordinal 2^32 on the device + 12345 {math}")


# ---- price_kernel and path_price_kernel ------------------------------------------------------------------------------
def _price(rows: np.ndarray, T: int, P: int, scheme: int, norm: int, ordinal0: int = ORD0) -> np.ndarray:
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    out = poisoned((rows.shape[0], _lib.PRICE_COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_price(_lib.ptr(cd), rows.shape[0], T, P, SEED, None, ordinal0, scheme, norm,
                                        _lib.DTYPE_F32, _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _price_paths(rows: np.ndarray, bars: np.ndarray, T: int, P: int, scheme: int, norm: int,
                 ordinal0: int = ORD0) -> np.ndarray:
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    bd = torch.tensor(bars, dtype=torch.float64, device=DEV)
    out = poisoned((rows.shape[0], _lib.PATH_PRICE_COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_price_paths(_lib.ptr(cd), _lib.ptr(bd), rows.shape[0], T, P, SEED, None, ordinal0,
                                              scheme, norm, _lib.DTYPE_F32, _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# (T, P, scheme): two whole chunks; odd T and a ragged P; the stream span at T = 1 and 2; T beyond one block of
# accumulator rows; one simple-Euler case
PRICE_CASES = [(16, 4096, LOG), (5, 693, LOG), (1, 528, LOG), (2, 1024, LOG), (40, 693, LOG), (5, 693, SIMPLE)]


@pytest.mark.parametrize("T,P,scheme", PRICE_CASES)
def test_price_kernel_columns(T, P, scheme) -> None:
    """smc_gbm_price raw, parked in LDS and replayed (forced with SMC_PRICE_REPLAY at these small P): the 8 columns,
    standard errors included."""
    name = _lib.lib().smc_gbm_price_kernel
    runs = inst.pricing_runs_of("price f32", (T, P, scheme))  # every launch the ledger counts for the row
    assert [r.name for r in runs] == 2 * ["price_kernel(raw)", "price_kernel(lds)", "price_kernel(replay)"]
    for math, (_, hw) in MATHS.items():
        for run in (r for r in runs if r.math == math):
            normalize, mode, flag = run.normalize, run.name[13:-1], (_lib.PRICE_REPLAY if run.force_replay else 0)
            assert name(T, P, scheme | hw | flag, int(normalize), _lib.DTYPE_F32).decode() == run.name
            rows, _ = case_rows(scheme, normalize)
            ref = _ref(12, T, P, scheme, normalize, math)
            got = _price(rows, T, P, scheme | hw | flag, int(normalize))
            label = f"price_kernel({mode}) T {T} P {P} {'log' if scheme == LOG else 'simple'} {math}"
            assert not np.isnan(got).any(), label
            used = {"means": gref.share_used(got[:, :3], ref.price[:, :3], ref.price_bound[:, :3]),
                    "stderr": gref.share_used(got[:, 3:5], ref.price[:, 3:5], ref.price_bound[:, 3:5]),
                    "intrinsic": gref.share_used(got[:, 5:7], ref.price[:, 5:7], ref.price_bound[:, 5:7]),
                    "terminal sum": gref.share_used(got[:, 7], ref.price[:, 7], ref.price_bound[:, 7])}
            print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
            assert max(used.values()) < 1.0, (label, used)
            if math == "portable":  # the terminal sum is the kernel mode's bit for bit: the CPU sweep's share
                _, _, krs = _oracle.kernel_paths(rows, T, P, SEED, ORD0, scheme)
                assert used["terminal sum"] == gref.share_used(krs[:, -1], ref.price[:, 7], ref.price_bound[:, 7]), label


@pytest.mark.parametrize("T,P,scheme", PRICE_CASES)
def test_path_price_kernel_columns(T, P, scheme) -> None:
    """smc_gbm_price_paths raw and replayed: the 20 columns, the knocked share under the count rule.  The barriers are
    about one standard deviation out (tests/test_gpu_path_price._barriers' rule), one contract has its upper barrier
    at the forward, inside the bulk, and the flat contract's sits on its paths where the bound is zero."""
    name = _lib.lib().smc_gbm_price_paths_kernel
    runs = inst.pricing_runs_of("path price f32", (T, P, scheme))  # every launch the ledger counts for the row
    assert [r.name for r in runs] == 2 * ["path_price_kernel(raw)", "path_price_kernel(replay)"]
    for math, (_, hw) in MATHS.items():
        for run in (r for r in runs if r.math == math):
            normalize, mode = run.normalize, run.name[18:-1]
            assert name(T, P, scheme | hw, int(normalize), _lib.DTYPE_F32).decode() == run.name
            rows, bars = case_rows(scheme, normalize)
            ref = _ref(12, T, P, scheme, normalize, math, bars=True)
            got = _price_paths(rows, bars, T, P, scheme | hw, int(normalize))
            label = f"path_price_kernel({mode}) T {T} P {P} {'log' if scheme == LOG else 'simple'} {math}"
            assert not np.isnan(got).any(), label
            means = [c for c in REST if c < 8 or c >= 16]
            used = {"means": gref.share_used(got[:, means], ref.path[:, means], ref.path_bound[:, means]),
                    "stderr": gref.share_used(got[:, 8:16], ref.path[:, 8:16], ref.path_bound[:, 8:16]),
                    "knocked share": gref.share_used(got[:, 17], ref.path[:, 17], ref.path_bound[:, 17])}
            print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
                  + f"; knocked share {ref.path[:, 17].min():.3f} .. {ref.path[:, 17].max():.3f}, "
                  f"paths in doubt {ref.doubt.tolist()}")
            assert used["knocked share"] <= 1.0, (label, used)  # a count: it may use its whole tolerance
            assert max(used["means"], used["stderr"]) < 1.0, (label, used)
