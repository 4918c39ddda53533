"""smc_gbm_greeks / smc_gbm_greeks_kernel on the host: argument errors come back as status codes before any
HIP call, the kernel choice follows the shape, and the binding's constants and the Python result types match
the header's column table.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import os
import re

from spectralmc_amd import _lib
from spectralmc_amd.gbm import BlackScholes

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
COLS = 26


def _greeks(L, contracts, B, T, P, scheme, norm, dtype, out) -> int:
    return int(L.smc_gbm_greeks(contracts, B, T, P, 7, None, 0, scheme, norm, dtype, out, None))


def test_greeks_argument_errors_do_not_launch() -> None:
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
    assert _greeks(L, p, 1, 16, 1024, 0x2000, 1, 0, p) == arg        # unknown flag
    assert "bad scheme" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, _lib.TRAIN_DYNAMIC, 1, 0, p) == arg  # another call's flag
    assert "bad scheme" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg
    assert "SMC_MATH_REF" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, _lib.MATH_REF | _lib.MATH_HW, 1, 0, p) == arg
    assert "SMC_MATH_REF" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, _lib.MATH_HW, 1, _lib.DTYPE_F64, p) == arg  # f64 has no HW math
    assert "f32 only" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 0, 7, 0, p) == arg             # bad normalization
    assert "normalization" in _lib.last_error()
    for flags in (0, _lib.MATH_HW, _lib.PRICE_REPLAY):               # simple Euler, in every math
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            assert _greeks(L, p, 1, 16, 1024, 1 | flags, norm, 0, p) == arg
            assert "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
    assert _greeks(L, p, 1, 16, 1024, 1, 1, _lib.DTYPE_F64, p) == arg
    assert "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
    for T, P, B in ((0, 1024, 1), (-3, 1024, 1), (16, 0, 1), (16, -8, 1), (16, 1024, -1), (16, 1 << 40, 1)):
        assert _greeks(L, p, B, T, P, 0, 1, 0, p) == shape
        assert "engine" in _lib.last_error()
    # the errors are checked before the empty batch is accepted
    assert _greeks(L, p, 0, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg
    assert _greeks(L, p, 0, 16, 1024, 1, 1, 0, p) == arg
    assert "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
    assert _greeks(L, p, 0, 16, 1024, 0, 1, 0, None) == arg
    assert _greeks(L, p, 0, 16, 1024, 0, 7, 0, p) == arg
    assert _greeks(L, p, 0, 0, 1024, 0, 1, 0, p) == shape
    assert all(v == 0.0 for v in dummy)


def test_greeks_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * COLS)(*([-1.5] * COLS))
    p = ctypes.addressof(dummy)
    for scheme in (0, _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.MATH_HW | _lib.PRICE_REPLAY):
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            assert _greeks(L, p, 0, 16, 1024, scheme, norm, 0, p) == _lib.SMC_OK
    assert _greeks(L, p, 0, 16, 1024, 0, 1, _lib.DTYPE_F64, p) == _lib.SMC_OK
    assert all(v == -1.5 for v in dummy)


def test_greeks_kernel_choice() -> None:
    L = _lib.lib()

    def name(T, P, scheme, norm, dtype) -> str:
        return L.smc_gbm_greeks_kernel(T, P, scheme, norm, dtype).decode()

    raw, norm = _lib.NORM_RAW, _lib.NORM_NORMALIZE
    f32, f64 = _lib.DTYPE_F32, _lib.DTYPE_F64
    for dtype in (f32, f64):
        for P in (1, 693, 4096, 1 << 20, (1 << 40) - 1):
            assert name(16, P, 0, raw, dtype) == "greeks_kernel(raw)"
    assert name(16, 4096, _lib.MATH_HW, raw, f32) == "greeks_kernel(raw)"
    assert name(16, 4096, 0, norm, f32) == "greeks_kernel(lds)"
    assert name(16, 4096, _lib.MATH_HW, norm, f32) == "greeks_kernel(lds)"
    assert name(3, 693, 0, norm, f32) == "greeks_kernel(lds)"
    assert name(16, 4096, 0, norm, f64) == "greeks_kernel(lds)"
    assert name(16, 1 << 20, 0, norm, f32) == "greeks_kernel(replay)"
    assert name(16, 65536, 0, norm, f32) == "greeks_kernel(replay)"
    assert name(16, 1 << 20, 0, norm, f64) == "greeks_kernel(replay)"
    # the flag forces replay at any NORMALIZE shape; RAW has one pass either way
    for P in (1, 528, 4096, 1 << 20):
        assert name(16, P, _lib.PRICE_REPLAY, norm, f32) == "greeks_kernel(replay)"
        assert name(16, P, _lib.PRICE_REPLAY | _lib.MATH_HW, norm, f32) == "greeks_kernel(replay)"
        assert name(16, P, _lib.PRICE_REPLAY, norm, f64) == "greeks_kernel(replay)"
    assert name(16, 4096, _lib.PRICE_REPLAY, raw, f32) == "greeks_kernel(raw)"
    # one switch point per element size: the parked row and the 320 B of pass-1 scratch in front of it stay
    # within 144 KiB, and with the f64 path math's 51,232 B static table image within a CU's 160 KiB of LDS
    for dtype, esz, fixed in ((f32, 4, 320), (f64, 8, 320 + 51232)):
        modes = [name(1, P, 0, norm, dtype) for P in range(1, 1 << 16)]
        edge = max(i for i, m in enumerate(modes) if m == "greeks_kernel(lds)") + 1
        assert modes[:edge] == ["greeks_kernel(lds)"] * edge
        assert modes[edge:] == ["greeks_kernel(replay)"] * (len(modes) - edge)
        parked = (edge * esz + 7) // 8 * 8
        assert 64 * 1024 <= parked and parked + 320 <= 144 * 1024 and parked + fixed <= 160 * 1024, (dtype, edge)
        # the price call parks the same contracts
        assert L.smc_gbm_price_kernel(1, edge, 0, norm, dtype) == b"price_kernel(lds)"
        assert L.smc_gbm_price_kernel(1, edge + 1, 0, norm, dtype) == b"price_kernel(replay)"
    # shapes and modes the call rejects
    for flags in (0, _lib.MATH_HW, _lib.PRICE_REPLAY):
        assert name(16, 4096, 1 | flags, norm, f32) == "unsupported"   # simple Euler
        assert name(16, 4096, 1 | flags, raw, f32) == "unsupported"
    assert name(16, 4096, 1, norm, f64) == "unsupported"
    assert name(16, 4096, _lib.MATH_REF, norm, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_REF, raw, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_HW, norm, f64) == "unsupported"
    assert name(16, 4096, 0, norm, 9) == "unsupported"
    assert name(0, 4096, 0, norm, f32) == "unsupported"
    assert name(-1, 4096, 0, norm, f32) == "unsupported"
    assert name(16, 0, 0, norm, f32) == "unsupported"
    assert name(16, -5, 0, norm, f32) == "unsupported"
    assert name(16, 4096, 5, norm, f32) == "unsupported"
    assert name(16, 4096, 0, 7, f32) == "unsupported"


NAMES = ["put_delta", "call_delta", "put_vega", "call_vega", "put_rho", "call_rho", "put_theta", "call_theta",
         "put_gamma", "call_gamma"]
FIELDS = NAMES + [n + "_stderr" for n in NAMES] + ["put_price", "call_price", "put_stderr", "call_stderr",
                                                    "terminal_sum", "terminal_log_sum"]


def test_greeks_constants_match_the_header() -> None:
    text = open(HEADER).read()

    def define(macro: str) -> int:
        return int(re.search(rf"#define\s+{macro}\s+(\w+)", text).group(1), 0)

    assert _lib.GREEKS_COLS == 26 == define("SMC_GREEKS_COLS")
    assert _lib.ABI_VERSION == define("SMC_ABI_VERSION") >= 19
    assert set(_lib.SIGNATURES) >= {"smc_gbm_greeks", "smc_gbm_greeks_kernel"}
    assert len(_lib.SIGNATURES["smc_gbm_greeks"][1]) == 12 and len(_lib.SIGNATURES["smc_gbm_greeks_kernel"][1]) == 5
    assert _lib.SIGNATURES["smc_gbm_greeks"] == _lib.SIGNATURES["smc_gbm_price"]
    assert _lib.SIGNATURES["smc_gbm_greeks_kernel"] == _lib.SIGNATURES["smc_gbm_price_kernel"]


def test_greeks_result_types_follow_the_column_table() -> None:
    assert len(FIELDS) == _lib.GREEKS_COLS
    assert list(BlackScholes.BatchGreeks.model_fields) == FIELDS
    assert list(BlackScholes.HostGreeks.model_fields) == FIELDS
    assert BlackScholes.HostGreeks.model_config.get("frozen") is True
    assert all(f.annotation is float for f in BlackScholes.HostGreeks.model_fields.values())
