"""smc_gbm_greeks_paths / smc_gbm_greeks_paths_kernel on the host: argument errors come back as status codes before
any HIP call and in the documented order, the kernel name follows the mode, the plan's sweep rows R and the bound on
the time steps are the header's, and the binding's constants and the Python result types match the header's column
table.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import os
import re
import subprocess
import sys

from spectralmc_amd import _lib
from spectralmc_amd.gbm import BlackScholes

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
COLS = 40
F64_TABLES = 51232  # the static table image of the f64 path math


def _greeks(L, contracts, B, T, P, scheme, norm, dtype, out) -> int:
    return int(L.smc_gbm_greeks_paths(contracts, B, T, P, 7, None, 0, scheme, norm, dtype, out, None))


def _plan(T: int, scheme: int, norm: int, dtype: int) -> tuple[int, int, int]:
    rows, lds = ctypes.c_int64(-7), ctypes.c_int64(-7)
    st = int(_lib.lib().smc_test_path_greeks_plan(T, scheme, norm, dtype, ctypes.byref(rows), ctypes.byref(lds)))
    return st, rows.value, lds.value


def test_path_greeks_argument_errors_do_not_launch_and_keep_their_order() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * COLS)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    assert _greeks(L, None, 1, 16, 1024, 0, 1, 0, p) == arg          # NULL contracts
    assert "contracts" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 0, 1, 0, None) == arg          # NULL output
    assert "greeks_dev" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 0, 1, 9, p) == arg             # bad dtype
    assert "dtype" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 5, 1, 0, p) == arg             # bad scheme
    assert "bad scheme" in _lib.last_error()
    for flag in (0x2000, _lib.TRAIN_DYNAMIC, _lib.PRICE_REPLAY):     # unknown bit, other calls' flags
        assert _greeks(L, p, 1, 16, 1024, flag, 1, 0, p) == arg
        assert "bad scheme" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg
    assert "SMC_MATH_REF" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, _lib.MATH_REF | _lib.MATH_HW, 1, 0, p) == arg
    assert "SMC_MATH_REF" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, _lib.MATH_HW, 1, _lib.DTYPE_F64, p) == arg  # f64 has no HW math
    assert "f32 only" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 0, 7, 0, p) == arg             # bad normalization
    assert "normalization" in _lib.last_error()
    for flags in (0, _lib.MATH_HW):                                  # simple Euler, in every math
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            assert _greeks(L, p, 1, 16, 1024, 1 | flags, norm, 0, p) == arg
            assert "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 1, 1, _lib.DTYPE_F64, p) == arg
    assert "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
    for T, P, B in ((0, 1024, 1), (-3, 1024, 1), (16, 0, 1), (16, -8, 1), (16, 1024, -1), (16, 1 << 40, 1)):
        assert _greeks(L, p, B, T, P, 0, 1, 0, p) == shape
        assert "engine" in _lib.last_error()
    # the order of smc_gbm_price_paths: the common shape checks, the output, the scheme, MATH_REF, HW with f64, the
    # normalisation, then simple Euler, then the bound on the time steps
    assert _greeks(L, None, 1, 0, 1024, 5, 7, 0, None) == arg and "contracts" in _lib.last_error()
    assert _greeks(L, p, 1, 0, 1024, 5, 7, 0, None) == shape and "engine" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 5, 7, 0, None) == arg and "greeks_dev" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 5, 7, 0, p) == arg and "bad scheme" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 1 | _lib.MATH_REF, 7, 0, p) == arg and "SMC_MATH_REF" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 1 | _lib.MATH_HW, 7, 1, p) == arg and "f32 only" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 1, 7, 0, p) == arg and "normalization" in _lib.last_error()
    assert _greeks(L, p, 1, 1 << 20, 1024, 1, 1, 0, p) == arg and "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
    assert _greeks(L, p, 1, 1 << 20, 1024, 0, 1, 0, p) == shape and "row tables" in _lib.last_error()
    # the errors are checked before the empty batch is accepted
    assert _greeks(L, p, 0, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg
    assert _greeks(L, p, 0, 16, 1024, 1, 1, 0, p) == arg
    assert "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
    assert _greeks(L, p, 0, 16, 1024, 0, 1, 0, None) == arg
    assert _greeks(L, p, 0, 16, 1024, 0, 7, 0, p) == arg
    assert _greeks(L, p, 0, 0, 1024, 0, 1, 0, p) == shape
    assert _greeks(L, p, 0, 1 << 20, 1024, 0, 0, 0, p) == shape
    assert all(v == 0.0 for v in dummy)


def test_path_greeks_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * COLS)(*([-1.5] * COLS))
    p = ctypes.addressof(dummy)
    for scheme in (0, _lib.MATH_HW):
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            assert _greeks(L, p, 0, 16, 1024, scheme, norm, 0, p) == _lib.SMC_OK
    assert _greeks(L, p, 0, 16, 1024, 0, 1, _lib.DTYPE_F64, p) == _lib.SMC_OK
    assert all(v == -1.5 for v in dummy)


def test_path_greeks_kernel_name() -> None:
    L = _lib.lib()

    def name(T, P, scheme, norm, dtype) -> str:
        return L.smc_gbm_greeks_paths_kernel(T, P, scheme, norm, dtype).decode()

    raw, norm = _lib.NORM_RAW, _lib.NORM_NORMALIZE
    f32, f64 = _lib.DTYPE_F32, _lib.DTYPE_F64
    for dtype in (f32, f64):
        for T in (1, 2, 5, 16, 29, 37, 1000):
            for P in (1, 693, 4096, 1 << 20, (1 << 40) - 1):
                assert name(T, P, 0, raw, dtype) == "path_greeks_kernel(raw)"
                assert name(T, P, 0, norm, dtype) == "path_greeks_kernel(replay)"
    assert name(16, 4096, _lib.MATH_HW, raw, f32) == "path_greeks_kernel(raw)"
    assert name(16, 4096, _lib.MATH_HW, norm, f32) == "path_greeks_kernel(replay)"
    # modes and shapes the call rejects
    for flags in (0, _lib.MATH_HW):
        assert name(16, 4096, 1 | flags, norm, f32) == "unsupported"   # simple Euler
        assert name(16, 4096, 1 | flags, raw, f32) == "unsupported"
    assert name(16, 4096, 1, norm, f64) == "unsupported"
    for flag in (_lib.MATH_REF, _lib.MATH_REF | _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.TRAIN_DYNAMIC, 0x2000):
        assert name(16, 4096, flag, norm, f32) == "unsupported"
        assert name(16, 4096, flag, raw, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_HW, norm, f64) == "unsupported"
    assert name(16, 4096, 0, norm, 9) == "unsupported"
    assert name(0, 4096, 0, norm, f32) == "unsupported"
    assert name(-1, 4096, 0, norm, f32) == "unsupported"
    assert name(16, 0, 0, norm, f32) == "unsupported"
    assert name(16, -5, 0, norm, f32) == "unsupported"
    assert name(16, 1 << 40, 0, norm, f32) == "unsupported"
    assert name(16, 4096, 5, norm, f32) == "unsupported"
    assert name(16, 4096, 0, 7, f32) == "unsupported"
    # the bound on the time steps, in both normalisations: the header's figures
    for dtype, last in ((f32, 8032), (f64, 2927)):
        for nm, label in ((raw, "raw"), (norm, "replay")):
            assert name(last, 4096, 0, nm, dtype) == f"path_greeks_kernel({label})"
            assert name(last + 1, 4096, 0, nm, dtype) == "unsupported"


def test_path_greeks_plan_rows_and_bound() -> None:
    """R from the header's rule: the LDS a workgroup may take (144 KiB in f32, 160 KiB less the table image in f64)
    less 2560 B of scratch and four tables of roundup8(T sizeof(Real)) bytes, over 8192 B per row pair, rounded
    down to even, and no more than T rounded up to even."""
    raw, norm = _lib.NORM_RAW, _lib.NORM_NORMALIZE
    ok, shape = _lib.SMC_OK, _lib.SMC_ERR_INVALID_SHAPE
    for dtype, esz, budget in ((_lib.DTYPE_F32, 4, 144 * 1024), (_lib.DTYPE_F64, 8, 160 * 1024 - F64_TABLES)):
        for T in (1, 2, 5, 12, 13, 16, 17, 29, 37, 48, 49, 1000, 2927):
            head = 2560 + 4 * ((T * esz + 7) // 8 * 8)
            fit = (budget - head) // 8192 // 2 * 2
            want = min((T + 1) // 2 * 2, fit)
            assert _plan(T, 0, norm, dtype) == (ok, want, head + want * 8192), (dtype, T)
            assert want >= 2 and want % 2 == 0 and head + want * 8192 <= budget
            assert _plan(T, 0, raw, dtype) == (ok, 0, head), (dtype, T)
    # the figures the header names, and the sweep counts the GPU tests rely on
    assert _plan(16, 0, norm, _lib.DTYPE_F32)[1] == 16 and _plan(16, 0, norm, _lib.DTYPE_F64)[1] == 12
    assert _plan(16, _lib.MATH_HW, norm, _lib.DTYPE_F32)[1] == 16
    assert _plan(37, 0, norm, _lib.DTYPE_F32)[1] == 16    # 16 + 16 + 5
    assert _plan(29, 0, norm, _lib.DTYPE_F64)[1] == 12    # 12 + 12 + 5
    assert _plan(5, 0, norm, _lib.DTYPE_F32)[1] == 6 and _plan(1, 0, norm, _lib.DTYPE_F64)[1] == 2
    # beyond the bound, and what the kernel does not take
    for dtype, last in ((_lib.DTYPE_F32, 8032), (_lib.DTYPE_F64, 2927)):
        for nm in (raw, norm):
            assert _plan(last, 0, nm, dtype)[0] == ok
            assert _plan(last + 1, 0, nm, dtype) == (shape, -7, -7)
    assert _plan(16, 1, norm, 0)[0] == shape and _plan(16, _lib.MATH_REF, norm, 0)[0] == shape
    assert _plan(16, _lib.MATH_HW, norm, _lib.DTYPE_F64)[0] == shape and _plan(16, 0, norm, 9)[0] == shape
    assert _plan(0, 0, norm, 0)[0] == shape
    L = _lib.lib()
    rows = ctypes.c_int64(0)
    assert L.smc_test_path_greeks_plan(16, 0, 1, 0, None, ctypes.byref(rows)) == _lib.SMC_ERR_INVALID_ARGUMENT
    assert L.smc_test_path_greeks_plan(16, 0, 1, 0, ctypes.byref(rows), None) == _lib.SMC_ERR_INVALID_ARGUMENT


def test_path_greeks_plan_hook_is_inert_without_the_environment_switch() -> None:
    """smc_test_path_greeks_plan writes nothing and fails unless SMC_ENABLE_TEST_HOOKS=1 (a fresh process without
    it, so this is its first hook call; no GPU call)."""
    code = ("import ctypes, sys; sys.path.insert(0, %r); from spectralmc_amd import _lib; L = _lib.lib(); "
            "a, b = ctypes.c_int64(-7), ctypes.c_int64(-7); "
            "print(L.smc_test_path_greeks_plan(16, 0, 1, 0, ctypes.byref(a), ctypes.byref(b)), _lib.last_error(), "
            "a.value, b.value)" % os.path.dirname(os.path.dirname(HEADER)))
    env = {k: v for k, v in os.environ.items() if k != "SMC_ENABLE_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[0] == str(_lib.SMC_ERR_INVALID_ARGUMENT) and "disabled" in out.stdout
    assert out.stdout.rstrip().endswith("-7 -7")


PAYOFFS = ["asian_put", "asian_call", "lookback_put", "lookback_call"]
NAMES = [f"{p}_{g}" for g in ("delta", "vega", "rho", "theta") for p in PAYOFFS]
FIELDS = NAMES + [n + "_stderr" for n in NAMES] + PAYOFFS + [p + "_stderr" for p in PAYOFFS]


def test_path_greeks_constants_and_symbols_match_the_header() -> None:
    text = open(HEADER).read()

    def define(macro: str) -> int:
        return int(re.search(rf"#define\s+{macro}\s+(\w+)", text).group(1), 0)

    assert _lib.PATH_GREEKS_COLS == COLS == define("SMC_PATH_GREEKS_COLS")
    assert _lib.ABI_VERSION == define("SMC_ABI_VERSION") == 21
    L = _lib.lib()
    assert hasattr(L, "smc_gbm_greeks_paths") and hasattr(L, "smc_gbm_greeks_paths_kernel")
    assert re.search(r"int32_t smc_gbm_greeks_paths\(const double\* contracts_dev, int64_t n_contracts, "
                     r"int32_t timesteps, int64_t n_paths,\s+uint64_t mc_seed, const int64_t\* ordinal_dev, "
                     r"int64_t ordinal0, int32_t scheme,\s+int32_t normalization, int32_t dtype, "
                     r"double\* greeks_dev /\*\[B\]\[40\]\*/, void\* stream\);", text)
    assert re.search(r"const char\* smc_gbm_greeks_paths_kernel\(int32_t timesteps, int64_t n_paths, int32_t scheme, "
                     r"int32_t normalization,\s+int32_t dtype\);", text)
    assert _lib.SIGNATURES["smc_gbm_greeks_paths"] == _lib.SIGNATURES["smc_gbm_greeks"]
    assert _lib.SIGNATURES["smc_gbm_greeks_paths_kernel"] == _lib.SIGNATURES["smc_gbm_greeks_kernel"]
    # the new section is the header's last, and the version comment gained its clause at the end only
    assert text.index("smc_gbm_greeks_paths(const") > text.index("smc_basket_price_paths_kernel(int32_t")
    line = next(ln for ln in text.splitlines() if ln.startswith("#define SMC_ABI_VERSION"))
    assert line.endswith("and so was smc_gbm_greeks_paths (with its _kernel query) */")


def test_path_greeks_result_types_follow_the_column_table() -> None:
    assert len(FIELDS) == _lib.PATH_GREEKS_COLS
    assert list(BlackScholes.PathBatchGreeks.model_fields) == FIELDS
    assert list(BlackScholes.HostPathGreeks.model_fields) == FIELDS
    assert BlackScholes.HostPathGreeks.model_config.get("frozen") is True
    assert all(f.annotation is float for f in BlackScholes.HostPathGreeks.model_fields.values())
