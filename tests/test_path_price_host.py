"""smc_gbm_price_paths / smc_gbm_price_paths_kernel on the host: argument errors come back as status codes
before any HIP call and before the empty batch is accepted, the kernel name follows the flags, and the
binding's constants match the header.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import os
import re

from spectralmc_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")


def _paths(L, contracts, barriers, B, T, P, scheme, norm, dtype, out) -> int:
    return int(L.smc_gbm_price_paths(contracts, barriers, B, T, P, 7, None, 0, scheme, norm, dtype, out, None))


def test_path_price_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 20)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    for bars in (None, p):
        assert _paths(L, None, bars, 1, 16, 1024, 0, 1, 0, p) == arg          # NULL contracts
        assert "contracts" in _lib.last_error()
        assert _paths(L, p, bars, 1, 16, 1024, 0, 1, 0, None) == arg          # NULL prices
        assert "prices_dev" in _lib.last_error()
        assert _paths(L, p, bars, 1, 16, 1024, 0, 1, 9, p) == arg             # bad dtype
        assert "dtype" in _lib.last_error()
        assert _paths(L, p, bars, 1, 16, 1024, 5, 1, 0, p) == arg             # bad scheme
        assert "scheme" in _lib.last_error()
        assert _paths(L, p, bars, 1, 16, 1024, 0x2000, 1, 0, p) == arg        # unknown flag
        assert _paths(L, p, bars, 1, 16, 1024, _lib.TRAIN_DYNAMIC, 1, 0, p) == arg  # other calls' flags
        assert _paths(L, p, bars, 1, 16, 1024, _lib.PRICE_REPLAY, 1, 0, p) == arg
        assert "scheme" in _lib.last_error()
        assert _paths(L, p, bars, 1, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg
        assert "SMC_MATH_REF" in _lib.last_error()
        assert _paths(L, p, bars, 1, 16, 1024, _lib.MATH_REF | _lib.MATH_HW, 1, 0, p) == arg
        assert _paths(L, p, bars, 1, 16, 1024, _lib.MATH_HW, 1, _lib.DTYPE_F64, p) == arg  # f64 has no HW math
        assert "f32 only" in _lib.last_error()
        assert _paths(L, p, bars, 1, 16, 1024, 0, 7, 0, p) == arg             # bad normalization
        assert "normalization" in _lib.last_error()
        assert _paths(L, p, bars, 1, 0, 1024, 0, 1, 0, p) == shape            # T <= 0
        assert _paths(L, p, bars, 1, -3, 1024, 0, 1, 0, p) == shape
        assert _paths(L, p, bars, 1, 16, 0, 0, 1, 0, p) == shape              # P <= 0
        assert _paths(L, p, bars, 1, 16, -8, 0, 1, 0, p) == shape
        assert _paths(L, p, bars, -1, 16, 1024, 0, 1, 0, p) == shape          # B < 0
        # more time steps than a workgroup's LDS holds row scales for (NORMALIZE only)
        assert _paths(L, p, bars, 1, 1 << 20, 1024, 0, 1, 0, p) == shape
        assert "timesteps" in _lib.last_error()
        # the errors are checked before the empty batch is accepted
        assert _paths(L, p, bars, 0, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg
        assert _paths(L, p, bars, 0, 16, 1024, 0, 1, 0, None) == arg
        assert _paths(L, p, bars, 0, 0, 1024, 0, 1, 0, p) == shape
    assert all(v == 0.0 for v in dummy)


def test_path_price_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 20)()
    p = ctypes.addressof(dummy)
    for dtype in (_lib.DTYPE_F32, _lib.DTYPE_F64):
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            for scheme in (0, 1) + ((_lib.MATH_HW, 1 | _lib.MATH_HW) if dtype == _lib.DTYPE_F32 else ()):
                for bars in (None, p):
                    for T in (1, 16, 40):
                        assert _paths(L, p, bars, 0, T, 1024, scheme, norm, dtype, p) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_path_price_kernel_names() -> None:
    L = _lib.lib()

    def name(T, P, scheme, norm, dtype) -> str:
        return L.smc_gbm_price_paths_kernel(T, P, scheme, norm, dtype).decode()

    raw, norm = _lib.NORM_RAW, _lib.NORM_NORMALIZE
    f32, f64 = _lib.DTYPE_F32, _lib.DTYPE_F64
    for dtype in (f32, f64):
        for scheme in (0, 1):
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20)):
                assert name(T, P, scheme, raw, dtype) == "path_price_kernel(raw)"
                assert name(T, P, scheme, norm, dtype) == "path_price_kernel(replay)"
    assert name(16, 4096, _lib.MATH_HW, norm, f32) == "path_price_kernel(replay)"
    assert name(16, 4096, 1 | _lib.MATH_HW, raw, f32) == "path_price_kernel(raw)"
    # flags, types and shapes the call rejects
    assert name(16, 4096, _lib.MATH_REF, norm, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_REF, raw, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_REF | _lib.MATH_HW, norm, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_HW, norm, f64) == "unsupported"
    assert name(16, 4096, _lib.PRICE_REPLAY, norm, f32) == "unsupported"
    assert name(16, 4096, _lib.TRAIN_DYNAMIC, norm, f32) == "unsupported"
    assert name(16, 4096, 0, norm, 9) == "unsupported"
    assert name(16, 4096, 5, norm, f32) == "unsupported"
    assert name(16, 4096, 0, 7, f32) == "unsupported"
    assert name(0, 4096, 0, norm, f32) == "unsupported"
    assert name(-1, 4096, 0, raw, f32) == "unsupported"
    assert name(16, 0, 0, norm, f32) == "unsupported"
    assert name(16, -4, 0, raw, f64) == "unsupported"
    # NORMALIZE keeps T row scales in LDS beside two accumulator rows at least: one switch point per dtype,
    # inside a CU's 160 KiB (f64: beside the 51,232 B static table image); RAW keeps nothing per row
    for dtype, esz, fixed in ((f32, 4, 0), (f64, 8, 51232)):
        names = [name(T, 4096, 0, norm, dtype) for T in range(1, 40000)]
        edge = max(i for i, m in enumerate(names) if m == "path_price_kernel(replay)") + 1
        assert names[:edge] == ["path_price_kernel(replay)"] * edge
        assert names[edge:] == ["unsupported"] * (len(names) - edge)
        assert edge >= 8192 and edge * esz + 20 * 8 * 8 + 2 * 4096 + fixed <= 160 * 1024, (dtype, edge)
        assert name(1 << 20, 4096, 0, raw, dtype) == "path_price_kernel(raw)"


def test_path_price_constants_match_the_header() -> None:
    text = open(HEADER).read()

    def define(macro: str) -> int:
        return int(re.search(rf"#define\s+{macro}\s+(\w+)", text).group(1), 0)

    assert _lib.PATH_PRICE_COLS == 20 == define("SMC_PATH_PRICE_COLS")
    assert _lib.ABI_VERSION == define("SMC_ABI_VERSION") >= 17
    assert set(_lib.SIGNATURES) >= {"smc_gbm_price_paths", "smc_gbm_price_paths_kernel"}
    assert len(_lib.SIGNATURES["smc_gbm_price_paths"][1]) == 13
    assert len(_lib.SIGNATURES["smc_gbm_price_paths_kernel"][1]) == 5
    assert _lib.SIGNATURES["smc_gbm_price_paths"][0] is ctypes.c_int32
    assert _lib.SIGNATURES["smc_gbm_price_paths_kernel"][0] is ctypes.c_char_p
    # the price call keeps its own shape
    assert _lib.PRICE_COLS == 8 and len(_lib.SIGNATURES["smc_gbm_price"][1]) == 12
