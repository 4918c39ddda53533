"""The reference-typing kernel (rows_ref_kernel, SMC_MATH_REF with portable and with hardware normals), every
Real = double kernel of csrc/gbm.hip and normalize_kernel against the independent reference of
tests/helpers/gbm_reference.py: every stored path element, row sum, target bin and price column within the a-priori
bound of the kernel's typing (REF_PORTABLE, REF_HW, F64_ENGINE; the f64 reference evaluated in long double), into
NaN-poisoned buffers, no element excluded.  The reference and its count condition are evaluated before the kernel's
output is looked at, each case asserts the name of the kernel it means to reach and prints the share of the bound it
uses, and a share below 1 everywhere is the only pass condition.  tests/test_gbm_typing_reference.py holds the CPU
stand-ins to the same references; the portable reference-typing cases assert that the stored paths use exactly the
share the oracle's MATH_REF kernel mode uses, which ties the two files.

The contracts are those of the CPU sweep (tests/test_gbm_reference.case_rows), repeated in order where a case needs
more than twelve."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from tests.helpers import gbm_reference as gref
from tests.helpers import instantiations as inst
from tests.helpers import poisoned
from tests.test_gbm_reference import REST, SEED, case_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
ORD0 = 3
ALL, TERMINAL, LOG, SIMPLE = _lib.STORE_ALL, _lib.STORE_TERMINAL, gref.LOG_EULER, gref.SIMPLE_EULER
F32, F64 = _lib.DTYPE_F32, _lib.DTYPE_F64
REF_MATHS = {"reference": (gref.REF_PORTABLE, _lib.MATH_REF),
             "reference_hw": (gref.REF_HW, _lib.MATH_REF | _lib.MATH_HW)}
F64_PARK = 14036  # the largest P whose f64 terminal row price_kernel parks in LDS (tests/test_gpu_greeks_reference.py)
needs_longdouble = pytest.mark.skipif(not gref.LONGDOUBLE_OK, reason="numpy.longdouble has no 64-bit significand here")


def _rows(B: int, scheme: int, normalize: bool) -> tuple[np.ndarray, np.ndarray]:
    rows, bars = case_rows(scheme, normalize)
    pick = np.arange(B) % rows.shape[0]
    return rows[pick], bars[pick]


@functools.lru_cache(maxsize=4)
def _ref(typing: str, B: int, T: int, P: int, scheme: int, normalize: bool, N: int = 0, M: int = 0, bars: bool = False,
         keep_paths: bool = False) -> gref.GbmRef:
    """The reference of the first B case rows in the typing, once per shape, with its count condition."""
    _oracle.build()
    ty = {"reference": gref.REF_PORTABLE, "reference_hw": gref.REF_HW, "f64": gref.F64_ENGINE,
          "f32": gref.F32_PORTABLE}[typing]
    rows, barriers = _rows(B, scheme, normalize)
    ref = gref.reference(_oracle, rows, T, P, SEED, ORD0, scheme=scheme, eps=ty, N=N, M=M, normalize=normalize,
                         bars=barriers if bars else None, keep_paths=keep_paths)
    if bars:
        assert gref.count_ok(ref.doubt, P), ref.doubt
    return ref


def _train_targets(rows: np.ndarray, T: int, N: int, M: int, scheme: int, normalize: bool, dtype: int, store: int,
                   pitch: int, *, with_rowsum: bool = False, sliced: bool = False):
    """(stored rows [B, T, P] or terminal rows [B, P], row sums [B, T] or None, targets [B, N]) of one smc_train_targets
    (scheme carries the math flags)."""
    L = _lib.lib()
    B, P = rows.shape[0], N * M
    real, cplx = (torch.float32, torch.complex64) if dtype == F32 else (torch.float64, torch.complex128)
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    paths = poisoned((B, T, pitch) if store == ALL else (B, pitch), real, DEV)
    rowsum = poisoned((B, T), torch.float64, DEV) if with_rowsum else None
    tg = poisoned((B, N), cplx, DEV)
    wsb = int(L.smc_engine_workspace_bytes(B, T, P, int(with_rowsum))) if sliced else 0
    assert not sliced or wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV) if sliced else None
    _lib.check(L.smc_train_targets(_lib.ptr(cd), B, T, N, M, SEED, None, ORD0, scheme, int(normalize), dtype, store,
                                   _lib.ptr(paths), pitch, B, _lib.ptr(rowsum), _lib.ptr(tg), _lib.ptr(ws), wsb, None))
    torch.cuda.synchronize()
    return paths[..., :P].cpu().numpy(), (rowsum.cpu().numpy() if with_rowsum else None), tg.cpu().numpy()


def _check_training(got: tuple, ref: gref.GbmRef, store: int, label: str) -> dict[str, float]:
    paths, rowsum, tg = got
    assert not np.isnan(paths).any() and not np.isnan(tg).any(), label
    want, bound = (ref.x, ref.dx) if store == ALL else (ref.xT, ref.dxT)
    used = {"paths": gref.share_used(paths, want, bound),
            "targets": gref.complex_share_used(tg, ref.targets, ref.targets_bound)}
    if rowsum is not None:
        assert not np.isnan(rowsum).any(), label
        used["row sums"] = gref.share_used(rowsum, ref.rowsum, ref.rowsum_bound)
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) < 1.0, (label, used)
    return used


def _label(kernel: str, T: int, N: int, M: int, scheme: int, normalize: bool, store: int, extra: str = "") -> str:
    return (f"{kernel} T {T} N {N} M {M} {'log' if scheme == LOG else 'simple'} {'NORM' if normalize else 'RAW'} "
            f"{'ALL' if store == ALL else 'TERMINAL'} {extra}").rstrip()


# ---- rows_ref_kernel + cf_kernel -------------------------------------------------------------------------------------
# (B, T, N, M, scheme, normalize, store)
REF_CASES = [
    (12, 16, 64, 64, LOG, True, ALL),         # whole chunks, an even T
    (12, 5, 100, 7, SIMPLE, True, ALL),       # P = 700: one partial chunk, the odd tail, simple Euler
    (12, 1, 16, 64, LOG, False, ALL),         # T = 1: the stream span, RAW
    (12, 33, 64, 16, LOG, True, TERMINAL),    # T > 16, terminal rows
    (4, 4, 99, 101, SIMPLE, True, TERMINAL),  # P = 9999: a lane straddles P
    (600, 3, 64, 32, LOG, True, ALL),         # more contracts than the persistent grid
    # the other cells of {log, simple} x {ALL, TERMINAL} at P = 700 and at P = 4096 (the eight instantiations
    # rows_ref_kernel<LOG_EULER, STORE_ALL, HWN> are each reached above as well: tests/test_instantiation_ledger.py)
    (12, 5, 100, 7, SIMPLE, True, TERMINAL),
    (12, 5, 100, 7, LOG, True, ALL),
    (12, 5, 100, 7, LOG, True, TERMINAL),
    (12, 16, 64, 64, LOG, True, TERMINAL),
    (12, 16, 64, 64, SIMPLE, True, ALL),
    (12, 16, 64, 64, SIMPLE, True, TERMINAL),
]


@pytest.mark.parametrize("B,T,N,M,scheme,normalize,store", REF_CASES)
def test_rows_ref_kernel_paths_and_targets(B, T, N, M, scheme, normalize, store) -> None:
    L = _lib.lib()
    P = N * M
    # rows_ref_kernel keeps the terminal sum in the row padding: the pitch of spectralmc_amd/engine.py, which leaves
    # room after column P where P itself is an odd multiple of 4 KiB (P = 1024)
    pitch = int(L.smc_path_pitch(P + 4, F32))
    rows, _ = _rows(B, scheme, normalize)
    for math, (_, flags) in REF_MATHS.items():
        query = F32 | flags | (0 if normalize else _lib.QUERY_RAW)
        assert L.smc_train_targets_kernel(T, N, P, query, pitch, 0) == b"rows_ref_kernel+cf_kernel"
        ref = _ref(math, B, T, P, scheme, normalize, N, M, keep_paths=True)
        got = _train_targets(rows, T, N, M, scheme | flags, normalize, F32, store, pitch)
        label = _label("rows_ref_kernel+cf_kernel", T, N, M, scheme, normalize, store, f"B {B} {math}")
        used = _check_training(got, ref, store, label)
        if math == "reference":  # bit for bit the oracle's MATH_REF kernel mode: the CPU sweep's share
            kp, term, _ = _oracle.kernel_paths(rows, T, P, SEED, ORD0, scheme | _oracle.MATH_REF, want_paths=True)
            kernel_mode = gref.share_used(kp, ref.x, ref.dx) if store == ALL else gref.share_used(term, ref.xT, ref.dxT)
            assert used["paths"] == kernel_mode, label


# ---- the f64 training kernels ----------------------------------------------------------------------------------------
# (kernel, B, T, N, M, scheme, normalize, store, padded pitch, sliced, also with row sums)
F64_TRAIN_CASES = [
    ("contract_kernel", 12, 7, 99, 7, SIMPLE, True, ALL, False, False, True),       # ragged P = 693, the odd tail
    ("contract_kernel", 12, 20, 100, 30, LOG, True, ALL, False, False, True),       # P = 3000, row-block replay
    ("rows_kernel+cf_kernel", 12, 17, 2048, 2, LOG, True, ALL, True, False, False),  # odd T beyond one row block
    ("rows_kernel+cf_kernel", 12, 3, 64, 96, LOG, True, ALL, True, False, False),    # P = 6144
    ("rows_kernel+cf_kernel", 12, 5, 128, 32, SIMPLE, False, TERMINAL, True, False, False),
    ("rows_kernel+cf_kernel", 12, 2, 64, 64, LOG, True, ALL, True, False, False),    # the stream span
    ("queue_kernel", 3, 16, 128, 80, LOG, True, ALL, False, True, False),            # sliced: P = 10,240 > 8192
    # ---- one row per instantiation (tests/test_instantiation_ledger.py) ----
    # rows_kernel<double>: P = 2048, within one row block and beyond it
    ("rows_kernel+cf_kernel", 12, 3, 64, 32, LOG, True, TERMINAL, True, False, False),
    ("rows_kernel+cf_kernel", 12, 3, 64, 32, SIMPLE, True, ALL, True, False, False),
    ("rows_kernel+cf_kernel", 12, 17, 64, 32, LOG, True, TERMINAL, True, False, False),
    ("rows_kernel+cf_kernel", 12, 17, 64, 32, SIMPLE, True, ALL, True, False, False),
    # queue_kernel<double> with row sums, and in simple Euler
    ("queue_kernel", 3, 4, 128, 80, LOG, True, ALL, False, True, True),
    ("queue_kernel", 3, 4, 128, 80, SIMPLE, True, ALL, False, True, True),
]


@needs_longdouble
@pytest.mark.parametrize("kernel,B,T,N,M,scheme,normalize,store,padded,sliced,rowsums", F64_TRAIN_CASES)
def test_f64_train_targets_paths_sums_and_targets(kernel, B, T, N, M, scheme, normalize, store, padded, sliced,
                                                  rowsums) -> None:
    L = _lib.lib()
    P = N * M
    pitch = int(L.smc_path_pitch(P, F64)) if padded else P
    query = F64 | (0 if normalize else _lib.QUERY_RAW)
    assert L.smc_train_targets_kernel(T, N, P, query, pitch, int(sliced)).decode() == kernel
    rows, _ = _rows(B, scheme, normalize)
    ref = _ref("f64", B, T, P, scheme, normalize, N, M, keep_paths=True)
    label = _label(kernel, T, N, M, scheme, normalize, store, "f64")
    got = _train_targets(rows, T, N, M, scheme, normalize, F64, store, pitch, sliced=sliced)
    _check_training(got, ref, store, label)
    if rowsums:
        got = _train_targets(rows, T, N, M, scheme, normalize, F64, store, pitch, sliced=sliced, with_rowsum=True)
        _check_training(got, ref, store, label + " with row sums")


def _simulate(rows: np.ndarray, T: int, P: int, scheme: int,
              dtype: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    paths = poisoned((rows.shape[0], T, P), torch.float32 if dtype == F32 else torch.float64, DEV)
    rowsum = poisoned((rows.shape[0], T), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_simulate(_lib.ptr(cd), rows.shape[0], T, P, SEED, None, ORD0, scheme, dtype,
                                           _lib.ptr(paths), _lib.ptr(rowsum), None))
    torch.cuda.synchronize()
    return cd, paths, rowsum


@needs_longdouble
@pytest.mark.parametrize("T,P", [(100, 64), (16, 4096)])
def test_f64_simulate_paths_and_row_sums(T, P) -> None:
    """smc_gbm_simulate in f64 with every row's sum: seven row blocks with step replay at a tiny P, and the
    straight 16-row block over two whole chunks."""
    rows, _ = _rows(12, LOG, True)
    ref = _ref("f64", 12, T, P, LOG, True, keep_paths=True)
    _, paths, rowsum = _simulate(rows, T, P, LOG, F64)
    got, rs = paths.cpu().numpy(), rowsum.cpu().numpy()
    assert not np.isnan(got).any() and not np.isnan(rs).any()
    used = {"paths": gref.share_used(got, ref.x, ref.dx), "row sums": gref.share_used(rs, ref.rowsum, ref.rowsum_bound)}
    print(f"smc_gbm_simulate f64 T {T} P {P}: share of the bound used "
          + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) < 1.0, used


# ---- normalize_kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,P", [(16, 4096), (5, 693)])
@pytest.mark.parametrize("typing,dtype", [("f32", F32), pytest.param("f64", F64, marks=needs_longdouble)])
def test_normalize_kernel_every_element(typing, dtype, T, P) -> None:
    """smc_gbm_simulate with row sums, then smc_gbm_normalize in place: every element against the reference's scaled
    rows x_t F_t / mean x_t and their bound (gbm_reference.scaled on gbm_reference.forwards)."""
    rows, _ = _rows(12, LOG, True)
    ref = _ref(typing, 12, T, P, LOG, True, keep_paths=True)
    fmt = gref.F64 if dtype == F64 else gref.F32
    F, eF = gref.forwards(rows, T, fmt=fmt)
    want, bound = gref.scaled(ref.x, ref.dx, ref.rowsum, ref.rowsum_bound, F, eF, fmt=fmt)
    cd, paths, rowsum = _simulate(rows, T, P, LOG, dtype)
    _lib.check(_lib.lib().smc_gbm_normalize(_lib.ptr(cd), 12, T, P, dtype, _lib.ptr(paths), _lib.ptr(rowsum), None))
    torch.cuda.synchronize()
    got = paths.cpu().numpy()
    assert not np.isnan(got).any()
    used = gref.share_used(got, want, bound)
    print(f"normalize_kernel {typing} T {T} P {P}: share of the bound used {used:.3f}")
    assert used < 1.0


# ---- f64 pricing -----------------------------------------------------------------------------------------------------
def _price(rows: np.ndarray, T: int, P: int, scheme: int, norm: int) -> np.ndarray:
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    out = poisoned((rows.shape[0], _lib.PRICE_COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_price(_lib.ptr(cd), rows.shape[0], T, P, SEED, None, ORD0, scheme, norm, F64,
                                        _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_price(got: np.ndarray, ref: gref.GbmRef, label: str) -> None:
    assert not np.isnan(got).any(), label
    used = {"means": gref.share_used(got[:, :3], ref.price[:, :3], ref.price_bound[:, :3]),
            "stderr": gref.share_used(got[:, 3:5], ref.price[:, 3:5], ref.price_bound[:, 3:5]),
            "intrinsic": gref.share_used(got[:, 5:7], ref.price[:, 5:7], ref.price_bound[:, 5:7]),
            "terminal sum": gref.share_used(got[:, 7], ref.price[:, 7], ref.price_bound[:, 7])}
    print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
    assert max(used.values()) < 1.0, (label, used)


# (T, P, scheme): tests/test_instantiation_ledger.py holds the two tables to the ledger of instantiations; the simple
# scheme's f64 instantiations have their row at the ragged shape
F64_PRICE_CASES = [(16, 4096, LOG), (5, 693, LOG), (5, 693, SIMPLE)]
F64_PATH_PRICE_CASES = [(16, 1024, LOG), (5, 693, LOG), (5, 693, SIMPLE)]


def _f64_price_kernel_columns(T: int, P: int, scheme: int) -> None:
    """Every launch the ledger counts for the row: raw, lds and forced replay."""
    name = _lib.lib().smc_gbm_price_kernel
    runs = inst.pricing_runs_of("price f64", (T, P, scheme))
    assert [r.name for r in runs] == ["price_kernel(raw)", "price_kernel(lds)", "price_kernel(replay)"]
    for run in runs:
        flag, normalize = (_lib.PRICE_REPLAY if run.force_replay else 0), run.normalize
        assert name(T, P, scheme | flag, int(normalize), F64).decode() == run.name
        rows, _ = _rows(12, scheme, normalize)
        ref = _ref("f64", 12, T, P, scheme, normalize)
        _check_price(_price(rows, T, P, scheme | flag, int(normalize)), ref,
                     f"{run.name} f64 T {T} P {P} {'log' if scheme == LOG else 'simple'}")


@needs_longdouble
@pytest.mark.parametrize("T,P", [c[:2] for c in F64_PRICE_CASES if c[2] == LOG])
def test_f64_price_kernel_columns(T, P) -> None:
    _f64_price_kernel_columns(T, P, LOG)


@needs_longdouble
@pytest.mark.parametrize("T,P", [c[:2] for c in F64_PRICE_CASES if c[2] == SIMPLE])
def test_f64_price_kernel_columns_simple_euler(T, P) -> None:
    _f64_price_kernel_columns(T, P, SIMPLE)


@needs_longdouble
def test_f64_price_kernel_replays_beyond_the_park_bound() -> None:
    """One path more than an f64 terminal row that fits in LDS: the shape itself selects the replay."""
    T, P, B = 2, F64_PARK + 1, 3
    name = _lib.lib().smc_gbm_price_kernel
    assert name(T, F64_PARK, LOG, 1, F64) == b"price_kernel(lds)" and name(T, P, LOG, 1, F64) == b"price_kernel(replay)"
    rows, _ = _rows(B, LOG, True)
    ref = _ref("f64", B, T, P, LOG, True)
    _check_price(_price(rows, T, P, LOG, 1), ref, f"price_kernel(replay) f64 T {T} P {P} B {B}")


def _f64_path_price_kernel_columns(T: int, P: int, scheme: int) -> None:
    """Every launch the ledger counts for the row: raw and the NORMALIZE replay."""
    name = _lib.lib().smc_gbm_price_paths_kernel
    runs = inst.pricing_runs_of("path price f64", (T, P, scheme))
    assert [r.name for r in runs] == ["path_price_kernel(raw)", "path_price_kernel(replay)"]
    for run in runs:
        normalize = run.normalize
        assert name(T, P, scheme, int(normalize), F64).decode() == run.name
        rows, bars = _rows(12, scheme, normalize)
        ref = _ref("f64", 12, T, P, scheme, normalize, bars=True)
        cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
        bd = torch.tensor(bars, dtype=torch.float64, device=DEV)
        out = poisoned((12, _lib.PATH_PRICE_COLS), torch.float64, DEV)
        _lib.check(_lib.lib().smc_gbm_price_paths(_lib.ptr(cd), _lib.ptr(bd), 12, T, P, SEED, None, ORD0, scheme,
                                                  int(normalize), F64, _lib.ptr(out), None))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        label = f"{run.name} f64 T {T} P {P} {'log' if scheme == LOG else 'simple'}"
        assert not np.isnan(got).any(), label
        means = [c for c in REST if c < 8 or c >= 16]
        used = {"means": gref.share_used(got[:, means], ref.path[:, means], ref.path_bound[:, means]),
                "stderr": gref.share_used(got[:, 8:16], ref.path[:, 8:16], ref.path_bound[:, 8:16]),
                "knocked share": gref.share_used(got[:, 17], ref.path[:, 17], ref.path_bound[:, 17])}
        print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
              + f"; paths in doubt {ref.doubt.tolist()}")
        assert used["knocked share"] <= 1.0, (label, used)  # a count: it may use its whole tolerance
        assert max(used["means"], used["stderr"]) < 1.0, (label, used)


@needs_longdouble
@pytest.mark.parametrize("T,P", [c[:2] for c in F64_PATH_PRICE_CASES if c[2] == LOG])
def test_f64_path_price_kernel_columns(T, P) -> None:
    _f64_path_price_kernel_columns(T, P, LOG)


@needs_longdouble
@pytest.mark.parametrize("T,P", [c[:2] for c in F64_PATH_PRICE_CASES if c[2] == SIMPLE])
def test_f64_path_price_kernel_columns_simple_euler(T, P) -> None:
    _f64_path_price_kernel_columns(T, P, SIMPLE)
