"""The instantiation ledger (tests/helpers/instantiations.py) against the source text of the dispatch and against the
case tables of the three float64-reference GPU files.  Three statements, none of which needs a GPU or the library:

* the ledger is what csrc/gbm.hip and csrc/basket.hip dispatch: the invocation lines of every SMC_* dispatch macro, the
  launch_rows_ref_k calls and the kernels each launch helper chooses between are read from the text and compared with
  the ledger, so an instantiation added to the source without a ledger entry fails here;
* every instantiation of the ledger that a call can reach is run by some row of TRAIN_CASES, REF_CASES,
  F64_TRAIN_CASES, SPLIT_CASES or RESIDENT_CASES (and the union holds nothing the ledger does not know), so an
  instantiation without a case, or a case row deleted that was the only one of its instantiation, fails here;
* the kernel name each case row states is the one the Python restatement of the host rules derives.  The GPU tests
  assert the stated name against the library's own name query, which ties the restatement to the library.
"""

from __future__ import annotations

import re
from collections import Counter
from itertools import product
from pathlib import Path

from tests.helpers import instantiations as inst
from tests.test_gpu_basket_reference import RESIDENT_CASES, SPLIT_CASES
from tests.test_gpu_gbm_reference import TRAIN_CASES
from tests.test_gpu_gbm_typing_reference import F64_TRAIN_CASES, REF_CASES

CSRC = Path(__file__).resolve().parents[1] / "spectralmc_amd" / "csrc"
TABLES = {"train": TRAIN_CASES, "ref": REF_CASES, "f64": F64_TRAIN_CASES, "basket split": SPLIT_CASES,
          "basket resident": RESIDENT_CASES}


def covered() -> dict[tuple, list[tuple[str, tuple]]]:
    """instantiation -> the (table, case row) pairs that run it."""
    runs: dict[tuple, list[tuple[str, tuple]]] = {}
    for table, cases in TABLES.items():
        for case in cases:
            for tup in inst.runs_of(table, case):
                runs.setdefault(tup, []).append((table, case))
    return runs


# ---- the ledger is what the source dispatches ------------------------------------------------------------------------
def _invocations(text: str, macro: str) -> list[tuple[bool, ...]]:
    """The argument lists of the macro's invocation lines (not its #define / #undef)."""
    lines = re.findall(rf"^\s*{macro}\(((?:true|false)(?:, (?:true|false))*)\)\s*$", text, flags=re.M)
    return [tuple(v == "true" for v in line.split(", ")) for line in lines]


def _scheme(le: bool) -> str:
    return "log" if le else "simple"


def _math(hw: bool) -> str:
    return "hw" if hw else "portable"


def _store(sa: bool) -> str:
    return "ALL" if sa else "TERMINAL"


def _of(kernel: str, dtype: str | None = None) -> set[tuple]:
    return {t for t in inst.ALL_GBM if t[0] == kernel and dtype in (None, t[1])}


def test_the_ledger_matches_the_dispatch_macros_of_gbm_hip() -> None:
    text = (CSRC / "gbm.hip").read_text()
    # the kernels each launch helper chooses between
    assert len(set(re.findall(r"wave_kernel<LOG_EULER, HW, STORE_ALL, (\d)>", text))) == len(inst.VARIANTS["wave_kernel"])
    assert (set(re.findall(r"(?<!_)resident_kernel<LOG_EULER, HW, STORE_ALL, ([a-z, ]+)>", text))
            == {"true", "false, true", "false"})  # T16, ONTHEFLY, rolled
    assert set(re.findall(r"packed_kernel<LOG_EULER, HW, STORE_ALL, ([a-z]+)>", text)) == {"true", "false"}
    by_macro = {m: _invocations(text, m) for m in ("SMC_WAVE", "SMC_RES", "SMC_PACK", "SMC_SPLIT", "SMC_ROWS", "SMC_LAUNCH")}
    for macro, lines in by_macro.items():
        assert len(lines) == len(set(lines)), f"{macro}: a repeated invocation line"
    for macro, kernel in (("SMC_WAVE", "wave_kernel"), ("SMC_RES", "resident_kernel"), ("SMC_PACK", "packed_kernel")):
        want = {(kernel, "f32", _scheme(le), _math(hw), _store(sa), v)
                for le, hw, sa in by_macro[macro] for v in inst.VARIANTS[kernel]}
        assert len(by_macro[macro]) * len(inst.VARIANTS[kernel]) == len(_of(kernel)), macro
        assert want == _of(kernel), macro
    want = {("paths_kernel", "f32", _scheme(le), _math(hw), _store(sa), "straight" if st else "split")
            for le, hw, st, sa in by_macro["SMC_SPLIT"]}
    assert len(by_macro["SMC_SPLIT"]) == len(_of("paths_kernel")) and want == _of("paths_kernel")
    # SMC_ROWS and SMC_LAUNCH: the HWM = true lines stand under if constexpr (sizeof(Real) == 4), and hw is false for
    # Real = double, so launch_engine<double> selects the HWM = false lines only
    rows = by_macro["SMC_ROWS"]
    assert {("rows_kernel", "f32", _scheme(le), _math(hw), _store(sa), "") for le, hw, sa in rows} == _of("rows_kernel", "f32")
    assert ({("rows_kernel", "f64", _scheme(le), "portable", _store(sa), "") for le, hw, sa in rows if not hw}
            == _of("rows_kernel", "f64"))
    assert len(rows) == len(_of("rows_kernel", "f32")) and sum(not hw for _, hw, _ in rows) == len(_of("rows_kernel", "f64"))
    launch = by_macro["SMC_LAUNCH"]
    for kernel in ("contract_kernel", "queue_kernel"):  # launch_engine_k: a.slices > 1 ? queue_kernel : contract_kernel
        assert ({(kernel, "f32", _scheme(le), _math(hw), "ROWSUMS" if ar else "NOSUMS", "") for le, hw, ar in launch}
                == _of(kernel, "f32"))
        assert ({(kernel, "f64", _scheme(le), "portable", "ROWSUMS" if ar else "NOSUMS", "") for le, hw, ar in launch if not hw}
                == _of(kernel, "f64"))
        assert len(launch) == len(_of(kernel, "f32")) and sum(not hw for _, hw, _ in launch) == len(_of(kernel, "f64"))
    assert len(re.findall(r"if constexpr \(sizeof\(Real\) == 4\) \{\n\s*SMC_(?:ROWS|LAUNCH)\(\w+, true, ", text)) == 2
    calls = re.findall(r"launch_rows_ref_k<(true|false), (true|false), (true|false)>\(a, stream\)", text)
    want = {("rows_ref_kernel", "f32", _scheme(le == "true"), "reference_hw" if hwn == "true" else "reference",
             _store(sa == "true"), "") for le, sa, hwn in calls}
    assert len(calls) == len(_of("rows_ref_kernel")) and want == _of("rows_ref_kernel")
    # nothing in the ledger beyond these, and no dispatch macro beyond these
    assert set(re.findall(r"^#define (SMC_[A-Z]+)\(", text, flags=re.M)) == set(by_macro)
    assert Counter(t[0] for t in inst.ALL_GBM) == {"wave_kernel": 16, "resident_kernel": 24, "packed_kernel": 16,
                                                   "paths_kernel": 12, "rows_kernel": 12, "contract_kernel": 12,
                                                   "queue_kernel": 12, "rows_ref_kernel": 8}


def test_the_ledger_matches_the_basket_dispatch() -> None:
    text = (CSRC / "basket.hip").read_text()
    assets = re.findall(r"case (\d): return f\(std::integral_constant<int, (\d)>\{\}\);", text)
    assert [int(a) for a, _ in assets] == [int(b) for _, b in assets] == list(range(1, inst.MAX_ASSETS + 1))
    assert set(re.findall(r"launch_per_contract\(basket_kernel<A, HW, (\d)>", text)) == {"0", "1"}
    assert set(re.findall(r"basket_resident_kernel<A, HW, (true|false)>", text)) == {"true", "false"}
    want = ({("basket_kernel", A, m, mode) for A, m, mode in product(range(1, 9), inst.MATHS, inst.BASKET_MODES)}
            | {("basket_resident_kernel", A, m, st) for A, m, st in product(range(1, 9), inst.MATHS, inst.STORES)})
    assert want == inst.ALL_BASKET
    # the constants of the resident kernel's LDS rule, which UNREACHABLE rests on
    assert "basket_resident_lds_bytes(A, static_cast<int>(N)) > 160 * 1024) return 0;" in text
    assert "constexpr int coef_stride(int A) { return 2 * A + A * A; }" in text
    assert [A for A in range(1, 9) if inst.basket_resident_lds_bytes(A) <= inst.BASKET_RES_LDS_LIMIT] == [1, 2, 3, 4, 5, 6]


def test_the_host_rule_constants_are_the_sources() -> None:
    text = (CSRC / "gbm.hip").read_text()
    for name, value in (("kThreads", 512), ("kPathsPerLane", 4), ("kSliceChunks", inst.K_SLICE_CHUNKS),
                        ("kRowBlock", inst.K_ROW_BLOCK), ("kResThreads", 1024), ("kResMaxChunks", inst.K_RES_MAX_CHUNKS),
                        ("kWaveMaxT", inst.K_WAVE_MAX_T)):
        assert re.search(rf"constexpr int {name} = {value};", text), name
    assert "constexpr int kPackMinP = 256, kPackMaxP = 2048;" in text
    assert inst.K_CHUNK == 512 * 4 and inst.K_RES_CHUNK == 1024 * 4 and inst.K_WAVE_CHUNK == 64 * inst.K_WAVE_LANE_PATHS
    assert inst.path_pitch(693) == 1024 and inst.path_pitch(1024) == 1024 and inst.path_pitch(1025) == 3072
    assert inst.path_pitch(4096, True) == 4608 and inst.slices_for(9999, True) == 2 and inst.slices_for(8192, True) == 1


# ---- every reachable instantiation has a case ------------------------------------------------------------------------
def test_every_reachable_instantiation_has_a_case() -> None:
    everything = inst.ALL_GBM | inst.ALL_BASKET
    assert set(inst.UNREACHABLE) <= everything and all(inst.UNREACHABLE.values())
    runs = covered()
    reachable = everything - set(inst.UNREACHABLE)
    print(f"instantiations {len(everything)} (single-asset {len(inst.ALL_GBM)}, basket {len(inst.ALL_BASKET)}), "
          f"reachable {len(reachable)}, covered {len(set(runs) & reachable)}")
    missing = sorted(map(str, reachable - set(runs)))
    assert not missing, f"no case row reaches: {missing}"
    unknown = sorted(map(str, set(runs) - reachable))
    assert not unknown, f"case rows reach what the ledger does not hold or calls unreachable: {unknown}"
    sole = sorted((len(v), str(k)) for k, v in runs.items() if len(v) == 1)
    print(f"{len(sole)} instantiations rest on a single case row")


def test_each_case_row_names_the_kernel_the_host_rules_derive() -> None:
    for table, cases in TABLES.items():
        assert len(set(cases)) == len(cases), f"{table}: a repeated case row"
        for case in cases:
            assert inst.derived_kernel(table, case) == inst.table_kernel(table, case), (table, case)
            for tup in inst.runs_of(table, case):  # with row sums no *_ok rule holds: contract_kernel or queue_kernel
                assert tup[0] in inst.table_kernel(table, case), (table, case, tup)
