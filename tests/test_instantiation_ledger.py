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

The same three statements hold for the batched pricing and Greeks kernels (ALL_GBM_PRICING, ALL_BASKET_PRICING): the
launch_*_k<Real, LOG_EULER, HW> selections, the ternaries over the modes, the slice passes and a.normalize,
with_price_mode, the pick(A, HW, MODE) callers and the constants of the park rules are read from the text; the tables
of PRICING_TABLES cover every instantiation; and the name of every launch inst.pricing_runs_of derives for a row is
what its GPU test asserts against the library's smc_*_kernel query, because those tests take their loops from it.
"""

from __future__ import annotations

import re
from collections import Counter
from itertools import product
from pathlib import Path

from tests.helpers import basket_general_cases, basket_general_greeks_cases, basket_greeks_cases
from tests.helpers import basket_path_cases, basket_path_greeks_cases
from tests.helpers import instantiations as inst
from tests.test_gpu_basket_reference import PRICE_CASES as BASKET_PRICE_CASES
from tests.test_gpu_basket_reference import LEDGER_PRICE_CASES, RESIDENT_CASES, SPLIT_CASES
from tests.test_gpu_gbm_reference import PRICE_CASES, TRAIN_CASES
from tests.test_gpu_gbm_typing_reference import F64_PATH_PRICE_CASES, F64_PRICE_CASES, F64_TRAIN_CASES, REF_CASES
from tests.test_gpu_greeks_reference import CASES as GREEKS_CASES
from tests.test_gpu_greeks_reference import F64_CASES as GREEKS_F64_CASES
from tests.test_gpu_path_greeks_reference import SHAPE_CASES as PATH_GREEKS_CASES
from tests.test_gpu_price_sliced import F64_SLICED_CASES, SLICED_CASES

CSRC = Path(__file__).resolve().parents[1] / "spectralmc_amd" / "csrc"
TABLES = {"train": TRAIN_CASES, "ref": REF_CASES, "f64": F64_TRAIN_CASES, "basket split": SPLIT_CASES,
          "basket resident": RESIDENT_CASES}
# the reference case tables of the batched pricing and Greeks kernels (inst.pricing_runs_of names their rows)
PRICING_TABLES = {
    "basket price": BASKET_PRICE_CASES, "basket general": basket_general_cases.CASES,
    "basket greeks": basket_greeks_cases.REFERENCE_CASES,
    "basket general greeks": basket_general_greeks_cases.REFERENCE_CASES,
    "basket path": basket_path_cases.CASES, "basket path greeks": basket_path_greeks_cases.CASES,
    "price f32": PRICE_CASES, "path price f32": PRICE_CASES, "price f64": F64_PRICE_CASES,
    "path price f64": F64_PATH_PRICE_CASES, "greeks f32": GREEKS_CASES, "greeks f64": GREEKS_F64_CASES,
    "path greeks": PATH_GREEKS_CASES, "sliced f32": SLICED_CASES, "sliced f64": F64_SLICED_CASES}


def covered() -> dict[tuple, list[tuple[str, tuple]]]:
    """instantiation -> the (table, case row) pairs that run it."""
    runs: dict[tuple, list[tuple[str, tuple]]] = {}
    for table, cases in TABLES.items():
        for case in cases:
            for tup in inst.runs_of(table, case):
                runs.setdefault(tup, []).append((table, case))
    for table, cases in PRICING_TABLES.items():
        for case in cases:
            for run in inst.pricing_runs_of(table, case):
                for tup in run.insts:
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


# ---- the pricing and Greeks ledger is what the source dispatches -----------------------------------------------------
HELPER_KERNELS = {"cf_kernel", "normalize_kernel", "normals_kernel", "advance_cursor_kernel", "basket_cf_kernel",
                  "basket_mean_fft_kernel"}  # no engine, pricing or Greeks template: outside the ledger
_B = {"true": True, "false": False}


def _body(text: str, signature: str) -> str:
    """The text of the host function whose first line holds `signature`, up to its closing brace in column 0."""
    start = text.index(signature)
    return text[start:text.index("\n}\n", start)]


def _gbm_pricing_from(text: str) -> set[tuple]:
    """ALL_GBM_PRICING as the text of gbm.hip dispatches it."""
    want: set[tuple] = set()
    # launch_X<Real>: the launch_X_k<Real, LOG_EULER, HW> (Greeks: <Real, HW>) selections; the HW ones stand under
    # if constexpr (sizeof(Real) == 4), so Real = double selects HW = false only
    typings = {}
    for helper, n_flags in (("price", 2), ("price_sliced", 2), ("path_price", 2), ("greeks", 1), ("path_greeks", 1)):
        body = _body(text, f"int32_t launch_{helper}(const EngineArgs& a")
        calls = re.findall(rf"launch_{helper}_k<Real((?:, (?:true|false))+)>\(", body)
        flags = [tuple(_B[v] for v in c.split(", ")[1:]) for c in calls]
        assert len(flags) == len(set(flags)) == 2 ** n_flags and all(len(f) == n_flags for f in flags), helper
        guard = body.index("if constexpr (sizeof(Real) == 4) {")
        close = body.index("\n  }\n", guard)
        for m in re.finditer(rf"launch_{helper}_k<Real((?:, (?:true|false))+)>\(", body):
            hw = m.group(1).endswith("true")
            assert (guard < m.start() < close) == hw, (helper, m.group(0))
        typings[helper] = [(d, (_scheme(f[0]) if n_flags == 2 else ""), _math(f[-1]))
                           for f in flags for d in (("f32", "f64") if not f[-1] else ("f32",))]
        assert len(re.findall(rf"launch_{helper}_k<", text)) == 2 ** n_flags, helper  # selected nowhere else
    # the kernels each launch_X_k chooses between
    modes = {"kPriceRaw": "raw", "kPriceLds": "lds", "kPriceReplay": "replay"}
    passes = {"kSliceRaw": "Raw", "kSliceSum": "Sum", "kSlicePay": "Pay"}
    norms = {"false": "RAW", "true": "NORMALIZE"}
    for kernel, helper, args, words in (
            ("price_kernel", "price", "Real, LOG_EULER, HW, ", modes),
            ("price_slice_kernel", "price_sliced", "Real, LOG_EULER, HW, ", passes),
            ("path_price_kernel", "path_price", "Real, LOG_EULER, HW, ", norms),
            ("greeks_kernel", "greeks", "Real, HW, ", modes),
            ("path_greeks_kernel", "path_greeks", "Real, HW, ", norms)):
        found = re.findall(rf"(?<![a-z_]){kernel}<([^<>]*)>", text)
        assert found and all(f.startswith(args) for f in found), kernel  # instantiated through its helper only
        last = {f[len(args):] for f in found}
        assert last == set(words), (kernel, last)
        want |= {(kernel, d, s, m, words[w]) for d, s, m in typings[helper] for w in last}
    assert set(re.findall(r"price_finish_kernel<(\w+)>", text)) == {"Real"}
    want |= {("price_finish_kernel", d, "", "portable", "") for d, _, _ in typings["price_sliced"]}
    return want


def test_the_pricing_ledger_matches_the_dispatch_of_gbm_hip() -> None:
    text = (CSRC / "gbm.hip").read_text()
    assert _gbm_pricing_from(text) == inst.ALL_GBM_PRICING
    assert Counter(t[0] for t in inst.ALL_GBM_PRICING) == {
        "price_kernel": 18, "price_slice_kernel": 18, "price_finish_kernel": 2, "path_price_kernel": 12,
        "greeks_kernel": 9, "path_greeks_kernel": 6}
    # the launch sequence of the sliced call, in stream order
    body = _body(text, "int32_t launch_price_sliced_k(const EngineArgs& a")
    launched = re.findall(r"launch\((price_slice_kernel<Real, LOG_EULER, HW, kSlice(\w+)>|price_finish_kernel<Real>)", body)
    assert [p or "finish" for _, p in launched] == ["Raw", "Sum", "finish", "Pay", "finish"]
    assert body.index("if (!a.normalize) {") < body.index("kSliceRaw") < body.index("} else {") < body.index("kSliceSum")
    assert body.index("kSlicePay") < body.index("\n  }\n") < body.rindex("launch(price_finish_kernel<Real>")
    for n in (False, True):
        seq = [t[4] or "finish" for t in inst.sliced_launches("f32", "log", "hw", n)]
        assert seq == (["Sum", "finish", "Pay", "finish"] if n else ["Raw", "finish"])
    # every __global__ of the two files is in a ledger, or a helper kernel without an engine's template arguments
    names = set(re.findall(r"__global__[^;{]*?\bvoid (\w+)\(", text + (CSRC / "basket.hip").read_text(), flags=re.S))
    ledgers = inst.ALL_GBM | inst.ALL_BASKET | inst.ALL_GBM_PRICING | inst.ALL_BASKET_PRICING
    assert names == {t[0] for t in ledgers} | HELPER_KERNELS


def _basket_pricing_from(text: str) -> set[tuple]:
    """ALL_BASKET_PRICING as the text of basket.hip dispatches it."""
    assets = [int(a) for a in re.findall(r"case (\d): return f\(std::integral_constant<int, \1>\{\}\);", text)]
    assert assets == list(range(1, inst.MAX_ASSETS + 1))
    assert "return on ? f(std::true_type{}) : f(std::false_type{});" in text  # with_flag: HW, NORM
    ternary = _body(text, "auto with_price_mode(int mode").split("{\n", 1)[1]  # past the signature's decltype
    modes = re.findall(r"f\(std::integral_constant<int, kBPrice(\w+)>\{\}\)", ternary)
    assert sorted(modes) == ["Lds", "Raw", "Replay"]
    enum = re.search(r"enum BasketPriceMode : int \{ kBPriceRaw = 0, kBPriceLds = 1, kBPriceReplay = 2 \};", text)
    assert enum, "BasketPriceMode"
    want: set[tuple] = set()
    picks = re.findall(r"\[\]\(auto A, auto HW, auto (MODE|NORM)\) \{ return (\w+)<A\(\), HW\(\), \1\(\)>; \};", text)
    assert len(picks) == len({k for _, k in picks}) == 6
    for arg, kernel in picks:
        # instantiated in its pick alone
        assert len(re.findall(rf"(?<![a-z_]){kernel}<", text)) == 1, kernel
        entry = _body(text, text[text.rindex("\nint32_t smc_", 0, text.index(f"return {kernel}<A()")) + 1:].split("(")[0] + "(")
        if arg == "MODE":
            assert re.search(r"return launch_parked\(c, kPark\w+, as_stream\(stream\), pick, ", entry), kernel
            want |= {(kernel, A, m, mode.lower()) for A, m, mode in product(assets, inst.MATHS, modes)}
        else:
            assert "return with_flag(a.normalize, [&](auto NORM) {" in entry and "pick(A, HW, NORM)" in entry, kernel
            want |= {(kernel, A, m, n) for A, m, n in product(assets, inst.MATHS, inst.NORMS)}
    # launch_parked: every (A, HW, MODE) of its kernel
    parked = _body(text, "int32_t launch_parked(const BasketCall& c")
    assert "with_variant(c.A, c.math & SMC_MATH_HW, c.entry, [&](auto A, auto HW) {" in parked
    assert "with_price_mode(mode, [&](auto MODE) {" in parked and "pick(A, HW, MODE)" in parked
    return want


def test_the_pricing_ledger_matches_the_basket_dispatch() -> None:
    text = (CSRC / "basket.hip").read_text()
    assert _basket_pricing_from(text) == inst.ALL_BASKET_PRICING
    assert Counter(t[0] for t in inst.ALL_BASKET_PRICING) == {
        **{k: 48 for k in inst.PARK_KERNELS}, **{k: 32 for k in inst.BASKET_PATH_KERNELS}}


def _flat(text: str) -> str:
    return re.sub(r"\s+", " ", text)


def test_the_park_rule_constants_are_the_sources() -> None:
    gbm, basket = _flat((CSRC / "gbm.hip").read_text()), _flat((CSRC / "basket.hip").read_text())
    # one parking bound in both files, the single-asset scratch, a CU's LDS
    for text in (gbm, basket):
        assert re.findall(r"#define SMC_PRICE_PARK_BYTES \((\d+) \* 1024\)", text) == [str(inst.PRICE_PARK_BYTES // 1024)]
    assert "constexpr size_t kPriceParkBytes = SMC_PRICE_PARK_BYTES;" in gbm
    assert "constexpr size_t kBPriceParkBytes = SMC_PRICE_PARK_BYTES;" in basket
    assert f"constexpr size_t kMaxLds = {inst.K_MAX_LDS // 1024} * 1024;" in gbm
    assert "constexpr int kPriceSums = 5;" in gbm and "constexpr int kWaves = kThreads / 64;" in gbm
    assert "constexpr size_t kPriceScratch = kWaves * kPriceSums * sizeof(double);" in gbm
    assert inst.K_PRICE_SCRATCH == 512 // 64 * 5 * 8
    for line in ("if (normalization == SMC_NORM_RAW) return kPriceRaw;", "if (scheme & SMC_PRICE_REPLAY) return kPriceReplay;",
                 "const size_t park = kPriceScratch + ((static_cast<size_t>(P) * esz + 7) & ~size_t{7});",
                 "const size_t fixed = dtype == SMC_DTYPE_F64 ? sizeof(math::F64Tables) : 0;",
                 "if (park > kPriceParkBytes || park + fixed > kMaxLds) return kPriceReplay;",
                 "const int mode = price_mode(P, scheme, normalization, dtype, lds);"):  # greeks_mode: price_mode's
        assert line in gbm, line
    # the park bounds the GPU tests hold the library to: the last P parked per element size
    assert [inst.price_mode(P, "f32", True) for P in (36784, 36785)] == ["lds", "replay"]
    assert [inst.price_mode(P, "f64", True) for P in (14036, 14037)] == ["lds", "replay"]  # F64_TABLE_BYTES
    assert inst.price_mode(1 << 30, "f32", False) == "raw" and inst.price_mode(1, "f64", True, True) == "replay"
    # the four ParkKernel constants: name, scratch
    parks = dict(re.findall(r'constexpr ParkKernel kPark\w+\{ ?"(\w+)", (\w+),', basket))
    assert parks == {"basket_price_kernel": "kBPriceScratch", "basket_general_kernel": "kBGeneralScratch",
                     "basket_greeks_kernel": "kBGreekScratch", "basket_greeks_general_kernel": "kBGGScratch"}
    assert set(parks) == set(inst.PARK_SCRATCH) == set(inst.PARK_KERNELS)
    for line in (
            "constexpr int kBWaves = kBThreads / 64;", "constexpr int kBThreads = 512;", "constexpr int kMaxAssets = 8;",
            "constexpr int kBPriceSums = 16;",
            "constexpr int kBPriceHead = kBWaves * kBPriceSums + kMaxAssets * kMaxAssets + kBWaves * kMaxAssets + kMaxAssets;",
            "constexpr size_t kBPriceScratch = kBPriceHead * sizeof(double);",
            "constexpr int kBGeneralHead = kBPriceHead;", "constexpr size_t kBGeneralScratch = kBGeneralHead * sizeof(double);",
            "constexpr int basket_greek_terms(int A) { return 4 * A + 8; }",
            "constexpr int kBGreekRed = 2 * basket_greek_terms(4);", "constexpr int kBGreekFc = 8;",
            "constexpr int kBGreekHead = kBWaves * kBGreekRed + 3 * kMaxAssets * kMaxAssets + kBWaves * 3 * kMaxAssets + "
            "3 * kMaxAssets + (kMaxAssets * kBGreekFc + kMaxAssets * kMaxAssets) / 2;",
            "constexpr size_t kBGreekScratch = kBGreekHead * sizeof(double);",
            "constexpr int basket_ggreek_pairs(int A) { return A * (A - 1) / 2; }",
            "constexpr int basket_ggreek_terms(int A) { return 4 * A + 6 + 2 * basket_ggreek_pairs(A); }",
            "constexpr int kBGGRed = 2 * basket_ggreek_terms(3);", "constexpr int kBGGMaxPairs = basket_ggreek_pairs(kMaxAssets);",
            "constexpr int kBGGSums = kMaxAssets + kMaxAssets * (kMaxAssets + 1) / 2;", "constexpr int kBGGFc = 8;",
            "constexpr int kBGGPc = kMaxAssets * kMaxAssets + 2 * kMaxAssets;",
            "constexpr int kBGGHead = kBWaves * kBGGRed + kMaxAssets * kMaxAssets + kBWaves * kBGGSums + kBGGSums + "
            "(kMaxAssets * kBGGFc + kBGGMaxPairs * kBGGPc) / 2;",
            "constexpr size_t kBGGScratch = kBGGHead * sizeof(double);",
            "static_assert(kBGGScratch == 15968 && kBGGScratch % 16 == 0",
            # basket_park_mode
            "*lds = k.scratch; if (normalization == SMC_NORM_RAW) return kBPriceRaw;",
            "if (math & SMC_PRICE_REPLAY) return kBPriceReplay;",
            "const size_t park = k.scratch + static_cast<size_t>(A) * ((static_cast<size_t>(P) + 3) & ~size_t{3}) * sizeof(float);",
            "if (park > kBPriceParkBytes) return kBPriceReplay;"):
        assert line in basket, line
    assert inst.PARK_SCRATCH == {"basket_price_kernel": 2112, "basket_general_kernel": 2112, "basket_greeks_kernel": 6848,
                                 "basket_greeks_general_kernel": 15968}
    # lds holds P = 693 for every A and kernel; the switch at A = 8 of the general Greeks (PARK_LAST, PARK_FIRST_REPLAY)
    assert all(inst.basket_park_mode(k, A, 693, True) == "lds" for k in inst.PARK_KERNELS for A in range(1, 9))
    assert [inst.basket_park_mode("basket_greeks_general_kernel", 8, P, True) for P in (4108, 4109)] == ["lds", "replay"]
    assert inst.basket_park_mode("basket_price_kernel", 2, 65536, True) == "replay"
    assert inst.basket_park_mode("basket_price_kernel", 4, 8192, True) == "lds"  # 128 KiB parked
    assert not inst.UNREACHABLE_PRICING


# ---- every reachable instantiation has a case ------------------------------------------------------------------------
def test_every_reachable_instantiation_has_a_case() -> None:
    training = inst.ALL_GBM | inst.ALL_BASKET
    pricing = inst.ALL_GBM_PRICING | inst.ALL_BASKET_PRICING
    assert not training & pricing and len(pricing) == 65 + 256
    everything = training | pricing
    unreachable = {**inst.UNREACHABLE, **inst.UNREACHABLE_PRICING}
    assert set(inst.UNREACHABLE) <= training and set(inst.UNREACHABLE_PRICING) <= pricing and all(unreachable.values())
    runs = covered()
    reachable = everything - set(unreachable)
    print(f"training instantiations {len(training)} (single-asset {len(inst.ALL_GBM)}, basket {len(inst.ALL_BASKET)}), "
          f"reachable {len(training & reachable)}, covered {len(set(runs) & training & reachable)}; "
          f"pricing and Greeks instantiations {len(pricing)} (single-asset {len(inst.ALL_GBM_PRICING)}, basket "
          f"{len(inst.ALL_BASKET_PRICING)}), reachable {len(pricing & reachable)}, covered "
          f"{len(set(runs) & pricing & reachable)}")
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
    for table, cases in PRICING_TABLES.items():
        assert len(set(cases)) == len(cases), f"{table}: a repeated case row"
        for case in cases:
            runs = inst.pricing_runs_of(table, case)
            assert runs and len({(r.math, r.dtype, r.normalize, r.force_replay) for r in runs}) == len(runs), (table, case)
            for run in runs:
                kernel, mode = run.insts[0][0], run.insts[0][-1]
                word = {"RAW": "raw", "NORMALIZE": "replay", "Raw": "raw", "Sum": "replay"}.get(mode, mode)
                assert run.name == f"{kernel}({word})", (table, case, run)
                assert not run.force_replay or (run.normalize and word == "replay"), (table, case, run)
            if table == "greeks f32":  # the row states its mode
                assert {r.insts[0][-1] for r in runs} == {case[0]}, case
    # the rows that state a park bound: the last P that parks and the first that replays
    gg = basket_general_greeks_cases
    assert [inst.basket_park_mode("basket_greeks_general_kernel", 8, P, True) for P in (gg.PARK_LAST, gg.PARK_FIRST_REPLAY)] \
        == ["lds", "replay"]


def test_each_row_at_the_ledger_shape_is_the_only_one_of_an_instantiation() -> None:
    """The rows added for the ledger (T = 3, P = 693, B = 3) are there for an (A, normalisation) no other row of their
    table reaches: each is the only row of at least one instantiation, so deleting any of them fails the test above."""
    runs = covered()
    added = {"basket price": LEDGER_PRICE_CASES, "basket general": basket_general_cases.LEDGER_CASES,
             "basket greeks": basket_greeks_cases.LEDGER_CASES, "basket general greeks": basket_general_greeks_cases.LEDGER_CASES,
             "basket path": basket_path_cases.LEDGER_CASES}
    assert [len(v) for v in added.values()] == [4, 11, 10, 9, 3]
    for table, cases in added.items():
        for case in cases:
            assert case in PRICING_TABLES[table] and {3, 693} <= set(case) and case[-1] == 3, (table, case)
            sole = [t for r in inst.pricing_runs_of(table, case) for t in r.insts if runs[t] == [(table, case)]]
            assert sole, (table, case)
