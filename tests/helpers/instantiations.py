"""The ledger of kernel instantiations: every template instantiation the host code of csrc/gbm.hip
(launch_engine<float>, launch_engine<double>) and csrc/basket.hip (launch_basket_k, launch_basket_resident_k) can
select for training, and (second half of the file: ALL_GBM_PRICING, ALL_BASKET_PRICING, pricing_runs_of) every one the
batched pricing and Greeks entries can select, written out literally, and the host rules that map a row of a
reference test's case table to the ones it runs.
tests/test_instantiation_ledger.py holds the ledger to the source text and the case tables to the ledger: the
unit that can be wrong in this code base is the instantiation, so every reachable one has to have
a case in the float64-reference files.  No GPU, no library: plain Python.

A single-asset tuple is (kernel, dtype, scheme, math, store, variant):
* kernel: the __global__ template's name;
* dtype "f32" / "f64", scheme "log" / "simple", math "portable" / "hw" (rows_ref_kernel: "reference" /
  "reference_hw", its HWN argument);
* store: the STORE_ALL template argument as "ALL" / "TERMINAL"; for contract_kernel and queue_kernel the ALLROWS
  argument as "ROWSUMS" / "NOSUMS" (their store mode is a run-time value);
* variant: what the launch helper selects beside the macro's arguments (launch_wave_k: "T1" / "T2";
  launch_resident_k: "T16" / "rolled" / "ONTHEFLY"; launch_packed_k: "T16" / "rolled"; SMC_SPLIT's ST argument:
  "straight" / "split"; "" elsewhere).
A basket tuple is (kernel, A, math, mode): basket_kernel's MODE as "fused" (0) / "split" (1, followed by
basket_cf_kernel), basket_resident_kernel's STORE_ALL as "ALL" / "TERMINAL".
"""

from __future__ import annotations

from dataclasses import dataclass
from itertools import product

SCHEMES = ("log", "simple")
MATHS = ("portable", "hw")
STORES = ("ALL", "TERMINAL")
SUMS = ("ROWSUMS", "NOSUMS")
REF_MATHS = ("reference", "reference_hw")
VARIANTS = {"wave_kernel": ("T1", "T2"), "resident_kernel": ("T16", "rolled", "ONTHEFLY"),
            "packed_kernel": ("T16", "rolled")}
# what smc_train_targets_kernel reports for the kernel
QUERY_NAME = {"wave_kernel": "wave_kernel", "resident_kernel": "resident_kernel", "packed_kernel": "packed_kernel",
              "paths_kernel": "paths_kernel+cf_kernel", "rows_kernel": "rows_kernel+cf_kernel",
              "rows_ref_kernel": "rows_ref_kernel+cf_kernel", "contract_kernel": "contract_kernel",
              "queue_kernel": "queue_kernel"}

ALL_GBM: frozenset[tuple] = frozenset(
    # SMC_WAVE x launch_wave_k's a.T == 1 ? <..., 1> : <..., 2>
    [("wave_kernel", "f32", s, m, st, v) for s, m, st, v in product(SCHEMES, MATHS, STORES, VARIANTS["wave_kernel"])]
    # SMC_RES x launch_resident_k's T == 16 ? T16 : (!normalize && W == 1) ? ONTHEFLY : rolled
    + [("resident_kernel", "f32", s, m, st, v)
       for s, m, st, v in product(SCHEMES, MATHS, STORES, VARIANTS["resident_kernel"])]
    # SMC_PACK x launch_packed_k's T == 16 ? T16 : rolled
    + [("packed_kernel", "f32", s, m, st, v) for s, m, st, v in product(SCHEMES, MATHS, STORES, VARIANTS["packed_kernel"])]
    # SMC_SPLIT: the straight form with either store, the other form with STORE_ALL = true only
    + [("paths_kernel", "f32", s, m, st, "straight") for s, m, st in product(SCHEMES, MATHS, STORES)]
    + [("paths_kernel", "f32", s, m, "ALL", "split") for s, m in product(SCHEMES, MATHS)]
    # SMC_ROWS: the HW lines under if constexpr (sizeof(Real) == 4)
    + [("rows_kernel", "f32", s, m, st, "") for s, m, st in product(SCHEMES, MATHS, STORES)]
    + [("rows_kernel", "f64", s, "portable", st, "") for s, st in product(SCHEMES, STORES)]
    # SMC_LAUNCH x launch_engine_k's a.slices > 1 ? queue_kernel : contract_kernel
    + [(k, "f32", s, m, rs, "") for k, s, m, rs in product(("contract_kernel", "queue_kernel"), SCHEMES, MATHS, SUMS)]
    + [(k, "f64", s, "portable", rs, "") for k, s, rs in product(("contract_kernel", "queue_kernel"), SCHEMES, SUMS)]
    # the eight launch_rows_ref_k<LOG_EULER, STORE_ALL, HWN> calls
    + [("rows_ref_kernel", "f32", s, m, st, "") for s, m, st in product(SCHEMES, REF_MATHS, STORES)])

MAX_ASSETS = 8
BASKET_MODES = ("fused", "split")
ALL_BASKET: frozenset[tuple] = frozenset(
    # with_variant (with_assets: A = 1..8, with_flag: HW) x launch_basket_k's MODE, launch_basket_resident_k's store_all
    [("basket_kernel", A, m, mode) for A, m, mode in product(range(1, MAX_ASSETS + 1), MATHS, BASKET_MODES)]
    + [("basket_resident_kernel", A, m, st) for A, m, st in product(range(1, MAX_ASSETS + 1), MATHS, STORES)])


# ---- the host rules of csrc/gbm.hip ----------------------------------------------------------------------------------
K_CHUNK, K_SLICE_CHUNKS, K_ROW_BLOCK = 2048, 4, 16
K_RES_CHUNK, K_RES_MAX_CHUNKS, K_RES_MAX_T = 4096, 16, 1 << 16
K_PACK_MIN_P, K_PACK_MAX_P = 256, 2048
K_WAVE_LANE_PATHS, K_WAVE_CHUNK, K_WAVE_MAX_T = 16, 1024, 2


def path_pitch(n_paths: int, f64: bool = False) -> int:
    """smc_path_pitch: the row rounded up to 4 KiB, then to an odd multiple of 4 KiB."""
    unit = 4096 // (8 if f64 else 4)
    units = -(-n_paths // unit)
    return (units + 1 - units % 2) * unit


def slices_for(P: int, sliced: bool) -> int:
    if not sliced:
        return 1
    return -(-(-(-P // K_CHUNK)) // K_SLICE_CHUNKS)


@dataclass(frozen=True)
class Args:
    """What the *_ok predicates read of EngineArgs in a smc_train_targets call (simulate and targets are set,
    res_slices is 0: whole contracts per resident workgroup)."""
    T: int
    N: int
    P: int
    pitch: int
    normalize: bool
    all_rows: bool
    slices: int
    f32: bool


def _pitch_ok(a: Args) -> bool:
    return a.pitch == 0 or (a.pitch % 4 == 0 and a.pitch >= a.P)


def wave_ok(a: Args) -> bool:
    return (a.f32 and not a.normalize and not a.all_rows and a.slices <= 1 and 1 <= a.T <= K_WAVE_MAX_T
            and a.P % K_WAVE_CHUNK == 0 and a.N >= K_WAVE_LANE_PATHS and a.N % K_WAVE_LANE_PATHS == 0
            and K_WAVE_CHUNK % a.N == 0 and _pitch_ok(a))


def resident_ok(a: Args) -> bool:
    return (a.f32 and not a.all_rows and a.slices <= 1 and 1 <= a.T <= K_RES_MAX_T and a.P % K_RES_CHUNK == 0
            and a.P // K_RES_CHUNK <= K_RES_MAX_CHUNKS and 4 <= a.N <= 1024 and K_RES_CHUNK % a.N == 0 and _pitch_ok(a))


def packed_ok(a: Args) -> bool:
    return (a.f32 and not a.all_rows and a.slices <= 1 and 1 <= a.T <= K_RES_MAX_T
            and K_PACK_MIN_P <= a.P <= K_PACK_MAX_P and K_RES_CHUNK % a.P == 0 and a.N >= 4 and a.N % 4 == 0
            and a.P % a.N == 0 and _pitch_ok(a))


def _padding(a: Args) -> int:
    return (a.pitch or a.P) - a.P


def split_ok(a: Args) -> bool:
    return a.f32 and not a.all_rows and a.slices <= 1 and _padding(a) >= (a.P & 1) + 2


def rows_ok(a: Args) -> bool:
    return (not a.all_rows and a.slices <= 1 and a.T >= 1 and a.P % K_CHUNK == 0
            and _padding(a) >= ((a.P & 1) + 2 if a.f32 else 1))


def ref_ok(a: Args) -> bool:
    return not a.all_rows and a.slices <= 1 and a.T >= 1 and _padding(a) >= (a.P & 1) + 2


def select(a: Args, reference_typing: bool = False) -> tuple[str, str]:
    """(kernel, variant) by launch_engine's order of precedence."""
    if reference_typing:
        assert a.f32 and ref_ok(a), "SMC_MATH_REF needs f32, whole contracts and a padded pitch"
        return "rows_ref_kernel", ""
    if a.f32:
        if wave_ok(a):
            return "wave_kernel", "T1" if a.T == 1 else "T2"
        if resident_ok(a):
            return "resident_kernel", "T16" if a.T == K_ROW_BLOCK else "rolled" if a.normalize else "ONTHEFLY"
        if packed_ok(a):
            return "packed_kernel", "T16" if a.T == K_ROW_BLOCK else "rolled"
        straight = a.T == K_ROW_BLOCK and a.P % K_CHUNK == 0
        if split_ok(a) and (straight or not rows_ok(a)):
            return "paths_kernel", "straight" if straight else "split"
    if rows_ok(a):
        return "rows_kernel", ""
    return ("queue_kernel" if a.slices > 1 else "contract_kernel"), ""


def gbm_instantiation(*, dtype: str, T: int, N: int, M: int, scheme: str, normalize: bool, store: str, pitch: int,
                      sliced: bool, with_rowsum: bool, math: str) -> tuple:
    P = N * M
    a = Args(T, N, P, pitch, normalize, with_rowsum, slices_for(P, sliced), dtype == "f32")
    kernel, variant = select(a, math in REF_MATHS)
    if kernel in ("contract_kernel", "queue_kernel"):
        store = "ROWSUMS" if with_rowsum else "NOSUMS"
    elif (kernel, variant) == ("paths_kernel", "split"):
        store = "ALL"  # SMC_SPLIT: (!ST || sa == SA), the one instantiation takes either run-time store mode
    return kernel, dtype, scheme, math, store, variant


# ---- the case tables -------------------------------------------------------------------------------------------------
_SCHEME = {0: "log", 1: "simple"}
_STORE = {2: "ALL", 1: "TERMINAL"}  # SMC_STORE_ALL, SMC_STORE_TERMINAL


def instantiation_of(table: str, case: tuple, math: str, with_rowsum: bool = False) -> tuple:
    """The instantiation one run of a case row reaches.  table: "train" (TRAIN_CASES of test_gpu_gbm_reference.py),
    "ref" (REF_CASES), "f64" (F64_TRAIN_CASES of test_gpu_gbm_typing_reference.py), "basket split" (SPLIT_CASES with
    math and with_rowsum = the terminal sums kept) or "basket resident" (RESIDENT_CASES with math and
    with_rowsum = every row stored)."""
    if table == "train":
        _, _, T, N, M, scheme, normalize, store, padded, sliced = case
        return gbm_instantiation(dtype="f32", T=T, N=N, M=M, scheme=_SCHEME[scheme], normalize=normalize,
                                 store=_STORE[store], pitch=path_pitch(N * M) if padded else N * M, sliced=sliced,
                                 with_rowsum=with_rowsum, math=math)
    if table == "ref":
        _, T, N, M, scheme, normalize, store = case
        return gbm_instantiation(dtype="f32", T=T, N=N, M=M, scheme=_SCHEME[scheme], normalize=normalize,
                                 store=_STORE[store], pitch=path_pitch(N * M + 4), sliced=False, with_rowsum=False,
                                 math=math)
    if table == "f64":
        _, _, T, N, M, scheme, normalize, store, padded, sliced, _ = case
        return gbm_instantiation(dtype="f64", T=T, N=N, M=M, scheme=_SCHEME[scheme], normalize=normalize,
                                 store=_STORE[store], pitch=path_pitch(N * M, True) if padded else N * M,
                                 sliced=sliced, with_rowsum=with_rowsum, math=math)
    if table == "basket split":
        A, T, N, M, _ = case
        assert basket_kernel_of(A, T, N, M, resident=False) == "basket_kernel"
        return "basket_kernel", A, math, "split" if with_rowsum else "fused"
    assert table == "basket resident", table
    A, N, M, _ = case
    assert basket_kernel_of(A, 16, N, M, resident=True) == "basket_resident_kernel"
    return "basket_resident_kernel", A, math, "ALL" if with_rowsum else "TERMINAL"


def runs_of(table: str, case: tuple) -> list[tuple]:
    """Every instantiation the test of the table runs for the case row: both math modes where the kernel has both, and
    contract_kernel / queue_kernel with and without row sums where the test asks for both."""
    if table == "train":
        sums = (False, True) if case[0] in ("contract_kernel", "queue_kernel") else (False,)
        return [instantiation_of(table, case, m, rs) for m in MATHS for rs in sums]
    if table == "ref":
        return [instantiation_of(table, case, m) for m in REF_MATHS]
    if table == "f64":
        return [instantiation_of(table, case, "portable", rs) for rs in ((False, True) if case[-1] else (False,))]
    return [instantiation_of(table, case, m, flag) for m in MATHS for flag in (False, True)]


def table_kernel(table: str, case: tuple) -> str:
    """The kernel name the case row states (what its GPU test asserts against the library's name query)."""
    return {"train": lambda: case[0], "f64": lambda: case[0], "ref": lambda: "rows_ref_kernel+cf_kernel",
            "basket split": lambda: "basket_kernel", "basket resident": lambda: "basket_resident_kernel"}[table]()


def derived_kernel(table: str, case: tuple) -> str:
    """The kernel name the host rules give for the case row's plain run, in the name query's words."""
    inst = runs_of(table, case)[0]
    return QUERY_NAME.get(inst[0], inst[0])


# ---- the host rules of csrc/basket.hip -------------------------------------------------------------------------------
K_R_CHUNK, K_R_MAX_SLICES, K_R_THREADS, K_R_WAVES, K_R_TABLE = 4096, 32, 1024, 16, 64
BASKET_RES_LDS_LIMIT = 160 * 1024


def basket_resident_lds_bytes(A: int) -> int:
    """basket_resident_lds_bytes: terminal slots [A][1024] of 16 B, part [4096] and wsum [16][8] and 16 more f64, two
    coefficient tables of 64 and two slots of [2 A + A^2] f32."""
    return A * K_R_THREADS * 16 + (4096 + K_R_WAVES * MAX_ASSETS + 16) * 8 + (2 * K_R_TABLE + 2) * (2 * A + A * A) * 4


def basket_res_slices(A: int, T: int, N: int, M: int) -> int:
    P = N * M
    if T != K_ROW_BLOCK or N < 4 or N > 2048 or N % 4 or K_R_CHUNK % N or P % K_R_CHUNK:
        return 0
    W = P // K_R_CHUNK
    return 0 if W < 1 or W > K_R_MAX_SLICES or basket_resident_lds_bytes(A) > BASKET_RES_LDS_LIMIT else W


def basket_kernel_of(A: int, T: int, N: int, M: int, *, resident: bool) -> str:
    return "basket_resident_kernel" if resident and basket_res_slices(A, T, N, M) > 0 else "basket_kernel"


# Instantiations the build contains and no call can reach, each with the host rule that keeps it out.
UNREACHABLE: dict[tuple, str] = {
    ("basket_resident_kernel", A, m, st):
        f"basket_res_slices returns 0: basket_resident_lds_bytes({A}, N) = {basket_resident_lds_bytes(A)} > 160 KiB for "
        "every N, so smc_basket_train_targets launches basket_kernel"
    for A, m, st in product((7, 8), MATHS, STORES)}


# ---- the batched pricing and Greeks kernels --------------------------------------------------------------------------
# A single-asset pricing tuple is (kernel, dtype, scheme, math, mode): scheme "" for the Greeks kernels (log-Euler
# only) and for price_finish_kernel<Real>; mode is the MODE argument "raw" / "lds" / "replay" (price_kernel,
# greeks_kernel), the PASS argument "Raw" / "Sum" / "Pay" (price_slice_kernel), the NORMALIZE argument "RAW" /
# "NORMALIZE" (path_price_kernel, path_greeks_kernel), "" for price_finish_kernel.  A basket pricing tuple is
# (kernel, A, math, mode) with the same words.
PRICE_MODES = ("raw", "lds", "replay")
SLICE_PASSES = ("Raw", "Sum", "Pay")
NORMS = ("RAW", "NORMALIZE")
# (dtype, math) of launch_price<Real> and its kin: the HW lines stand under if constexpr (sizeof(Real) == 4)
TYPINGS = (("f32", "portable"), ("f32", "hw"), ("f64", "portable"))

ALL_GBM_PRICING: frozenset[tuple] = frozenset(
    # launch_price_k<Real, LOG_EULER, HW> x its ternary over kPriceRaw / kPriceLds / kPriceReplay
    [("price_kernel", d, s, m, mode) for (d, m), s, mode in product(TYPINGS, SCHEMES, PRICE_MODES)]
    # launch_price_sliced_k<Real, LOG_EULER, HW>: kSliceRaw, or kSliceSum and kSlicePay, and price_finish_kernel<Real>
    + [("price_slice_kernel", d, s, m, ps) for (d, m), s, ps in product(TYPINGS, SCHEMES, SLICE_PASSES)]
    + [("price_finish_kernel", d, "", "portable", "") for d in ("f32", "f64")]
    # launch_path_price_k<Real, LOG_EULER, HW> x a.normalize
    + [("path_price_kernel", d, s, m, n) for (d, m), s, n in product(TYPINGS, SCHEMES, NORMS)]
    # launch_greeks_k<Real, HW> x its ternary over the three modes; launch_path_greeks_k<Real, HW> x a.normalize
    + [("greeks_kernel", d, "", m, mode) for (d, m), mode in product(TYPINGS, PRICE_MODES)]
    + [("path_greeks_kernel", d, "", m, n) for (d, m), n in product(TYPINGS, NORMS)])

PARK_KERNELS = ("basket_price_kernel", "basket_general_kernel", "basket_greeks_kernel", "basket_greeks_general_kernel")
BASKET_PATH_KERNELS = ("basket_path_kernel", "basket_path_greeks_kernel")
ALL_BASKET_PRICING: frozenset[tuple] = frozenset(
    # launch_parked: with_variant (A = 1..8, HW) x with_price_mode, for each pick(A, HW, MODE) caller
    [(k, A, m, mode) for k, A, m, mode in product(PARK_KERNELS, range(1, MAX_ASSETS + 1), MATHS, PRICE_MODES)]
    # with_variant x with_flag(a.normalize)
    + [(k, A, m, n) for k, A, m, n in product(BASKET_PATH_KERNELS, range(1, MAX_ASSETS + 1), MATHS, NORMS)])

# No host rule keeps a pricing or Greeks instantiation out: SMC_PRICE_REPLAY reaches replay at any P, and the parked
# block of P = 693 paths fits for every A.
UNREACHABLE_PRICING: dict[tuple, str] = {}

# ---- the park rule: price_mode / greeks_mode (gbm.hip) and basket_park_mode (basket.hip) ----
PRICE_PARK_BYTES = 144 * 1024      # SMC_PRICE_PARK_BYTES in both files
K_MAX_LDS = 160 * 1024             # kMaxLds
K_PRICE_SCRATCH = 8 * 5 * 8        # kPriceScratch = kWaves * kPriceSums * sizeof(double)
F64_TABLE_BYTES = 51232            # sizeof(math::F64Tables): the static LDS image of the f64 path math
K_B_WAVES = 8                      # kBWaves = kBThreads / 64


def _greek_terms(A: int) -> int:   # basket_greek_terms
    return 4 * A + 8


def _ggreek_terms(A: int) -> int:  # basket_ggreek_terms
    return 4 * A + 6 + A * (A - 1)


_M = MAX_ASSETS
K_B_PRICE_HEAD = K_B_WAVES * 16 + _M * _M + K_B_WAVES * _M + _M                      # kBPriceHead, kBPriceSums = 16
K_B_GREEK_HEAD = (K_B_WAVES * 2 * _greek_terms(4) + 3 * _M * _M + K_B_WAVES * 3 * _M + 3 * _M
                  + (_M * 8 + _M * _M) // 2)                                         # kBGreekHead, kBGreekFc = 8
_GG_SUMS = _M + _M * (_M + 1) // 2                                                   # kBGGSums
K_B_GG_HEAD = (K_B_WAVES * 2 * _ggreek_terms(3) + _M * _M + K_B_WAVES * _GG_SUMS + _GG_SUMS
               + (_M * 8 + (_M * (_M - 1) // 2) * (_M * _M + 2 * _M)) // 2)          # kBGGHead, kBGGFc = 8
# the scratch member of each ParkKernel constant, in bytes
PARK_SCRATCH = {"basket_price_kernel": 8 * K_B_PRICE_HEAD, "basket_general_kernel": 8 * K_B_PRICE_HEAD,
                "basket_greeks_kernel": 8 * K_B_GREEK_HEAD, "basket_greeks_general_kernel": 8 * K_B_GG_HEAD}


def price_mode(P: int, dtype: str, normalize: bool, force_replay: bool = False) -> str:
    """price_mode and greeks_mode of gbm.hip: the scratch and the terminal row of P Reals (padded to 8 B) are parked
    while they fit SMC_PRICE_PARK_BYTES and, beside the f64 kernels' static tables, a CU's LDS."""
    if not normalize:
        return "raw"
    if force_replay:
        return "replay"
    esz, fixed = (8, F64_TABLE_BYTES) if dtype == "f64" else (4, 0)
    park = K_PRICE_SCRATCH + (P * esz + 7) // 8 * 8
    return "replay" if park > PRICE_PARK_BYTES or park + fixed > K_MAX_LDS else "lds"


def basket_park_mode(kernel: str, A: int, P: int, normalize: bool, force_replay: bool = False) -> str:
    """basket_park_mode of basket.hip: the kernel's scratch and [A][P rounded up to 4] floats against kBPriceParkBytes."""
    if not normalize:
        return "raw"
    if force_replay:
        return "replay"
    return "replay" if PARK_SCRATCH[kernel] + A * ((P + 3) // 4 * 4) * 4 > PRICE_PARK_BYTES else "lds"


def sliced_launches(dtype: str, scheme: str, math: str, normalize: bool) -> list[tuple]:
    """launch_price_sliced_k's launches in stream order: RAW runs Raw then finish; NORMALIZE runs Sum, finish (totals
    only), Pay, finish."""
    finish = ("price_finish_kernel", dtype, "", "portable", "")
    if not normalize:
        return [("price_slice_kernel", dtype, scheme, math, "Raw"), finish]
    return [("price_slice_kernel", dtype, scheme, math, "Sum"), finish,
            ("price_slice_kernel", dtype, scheme, math, "Pay"), finish]


@dataclass(frozen=True)
class Run:
    """One launch (one call, for the sliced entry) a reference test makes for a case row and holds to the float64
    reference: the instantiations it runs (the first is the one the name query reports), the flags of the call and
    the name its smc_*_kernel query must give."""
    insts: tuple[tuple, ...]
    math: str          # "portable" / "hw"
    dtype: str         # "f32" / "f64" (basket: "f32")
    normalize: bool
    force_replay: bool  # SMC_PRICE_REPLAY set in the call
    name: str


def _park_run(kernel: str, A: int, P: int, math: str, normalize: bool, force: bool) -> Run:
    mode = basket_park_mode(kernel, A, P, normalize, force)
    return Run(((kernel, A, math, mode),), math, "f32", normalize, force, f"{kernel}({mode})")


def park_runs(kernel: str, A: int, P: int, normalize: bool, maths: tuple[str, ...] = MATHS) -> list[Run]:
    """Both maths; the mode the shape selects and, where that is lds, SMC_PRICE_REPLAY's replay as well."""
    out = []
    for m in maths:
        out.append(_park_run(kernel, A, P, m, normalize, False))
        if out[-1].insts[0][3] == "lds":
            out.append(_park_run(kernel, A, P, m, normalize, True))
    return out


def _basket_path_runs(kernel: str, A: int) -> list[Run]:
    return [Run(((kernel, A, m, NORMS[n]),), m, "f32", bool(n), False, f"{kernel}({'replay' if n else 'raw'})")
            for m in MATHS for n in (1, 0)]


def _price_runs(kernel: str, dtype: str, scheme: str, P: int, maths: tuple[str, ...], norms=(False, True)) -> list[Run]:
    """price_kernel / greeks_kernel: per math raw, the mode the shape selects and, where that is lds, forced replay."""
    out = []
    for m in maths:
        for normalize in norms:
            for force in ((False, True) if normalize and price_mode(P, dtype, True) == "lds" else (False,)):
                mode = price_mode(P, dtype, normalize, force)
                out.append(Run(((kernel, dtype, scheme, m, mode),), m, dtype, normalize, force, f"{kernel}({mode})"))
    return out


def _path_runs(kernel: str, dtype: str, scheme: str, maths: tuple[str, ...], norms=(False, True)) -> list[Run]:
    return [Run(((kernel, dtype, scheme, m, NORMS[n]),), m, dtype, n, False, f"{kernel}({'replay' if n else 'raw'})")
            for m in maths for n in norms]


def _sliced_runs(dtype: str, scheme: str, maths: tuple[str, ...]) -> list[Run]:
    return [Run(tuple(sliced_launches(dtype, scheme, m, n)), m, dtype, n, False,
                f"price_slice_kernel({'replay' if n else 'raw'})") for m in maths for n in (False, True)]


def pricing_runs_of(table: str, case: tuple) -> list[Run]:
    """Every launch the reference test of the table makes for the case row.  The GPU tests take their loops from here,
    so a row cannot claim an instantiation its test does not launch and compare.  Tables:
    basket price (A, T, P, B)                 PRICE_CASES of tests/test_gpu_basket_reference.py, both normalisations
    basket general (A, T, P, norm, B)         basket_general_cases.CASES
    basket greeks (A, T, P, norm, B)          basket_greeks_cases.REFERENCE_CASES
    basket general greeks (kind, A, T, P, norm, B)  basket_general_greeks_cases.REFERENCE_CASES
    basket path, basket path greeks (A, T, P, B)    basket_path_cases.CASES, basket_path_greeks_cases.CASES
    price f32, path price f32 (T, P, scheme)  PRICE_CASES of tests/test_gpu_gbm_reference.py
    price f64, path price f64 (T, P, scheme)  F64_PRICE_CASES, F64_PATH_PRICE_CASES of test_gpu_gbm_typing_reference.py
    greeks f32 (mode, B, T, P, force_replay)  CASES of tests/test_gpu_greeks_reference.py; greeks f64 (T, P) F64_CASES
    path greeks (math, T, P)                  SHAPE_CASES of tests/test_gpu_path_greeks_reference.py
    sliced f32 (T, P, span, scheme), sliced f64 (T, P, span, scheme)  of tests/test_gpu_price_sliced.py"""
    if table == "basket price":
        A, _, P, _ = case
        return [r for n in (False, True) for r in park_runs("basket_price_kernel", A, P, n)]
    if table in ("basket general", "basket greeks"):
        A, _, P, norm, _ = case
        return park_runs("basket_general_kernel" if table == "basket general" else "basket_greeks_kernel", A, P, bool(norm))
    if table == "basket general greeks":
        _, A, _, P, norm, _ = case
        return park_runs("basket_greeks_general_kernel", A, P, bool(norm))
    if table == "basket path":
        return _basket_path_runs("basket_path_kernel", case[0])
    if table == "basket path greeks":
        return _basket_path_runs("basket_path_greeks_kernel", case[0])
    if table in ("price f32", "price f64"):
        _, P, scheme = case
        d = table[-3:]
        return _price_runs("price_kernel", d, _SCHEME[scheme], P, MATHS if d == "f32" else ("portable",))
    if table in ("path price f32", "path price f64"):
        d = table[-3:]
        return _path_runs("path_price_kernel", d, _SCHEME[case[2]], MATHS if d == "f32" else ("portable",))
    if table == "greeks f32":
        mode, _, _, P, force = case
        normalize = mode != "raw"
        return [Run((("greeks_kernel", "f32", "", m, price_mode(P, "f32", normalize, bool(force))),), m, "f32", normalize,
                    bool(force), f"greeks_kernel({price_mode(P, 'f32', normalize, bool(force))})") for m in MATHS]
    if table == "greeks f64":
        return _price_runs("greeks_kernel", "f64", "", case[1], ("portable",))
    if table == "path greeks":
        math = case[0]
        return _path_runs("path_greeks_kernel", "f64" if math == "f64" else "f32", "", ("portable" if math == "f64" else math,))
    if table in ("sliced f32", "sliced f64"):
        d = table[-3:]
        return _sliced_runs(d, _SCHEME[case[3]], MATHS if d == "f32" else ("portable",))
    raise AssertionError(table)
