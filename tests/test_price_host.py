"""smc_gbm_price / smc_gbm_price_kernel on the host: argument errors come back as status codes before any
HIP call, the kernel choice follows the shape, and the binding's constants match the header.  CPU only
(no kernel launches)."""

from __future__ import annotations

import ctypes
import os
import re

from spectralmc_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")


def _price(L, contracts, B, T, P, scheme, norm, dtype, out) -> int:
    return int(L.smc_gbm_price(contracts, B, T, P, 7, None, 0, scheme, norm, dtype, out, None))


def test_price_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 8)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    assert _price(L, None, 1, 16, 1024, 0, 1, 0, p) == arg          # NULL contracts
    assert "contracts" in _lib.last_error()
    assert _price(L, p, 1, 16, 1024, 0, 1, 0, None) == arg          # NULL prices
    assert "prices_dev" in _lib.last_error()
    assert _price(L, p, 1, 16, 1024, 0, 1, 9, p) == arg             # bad dtype
    assert _price(L, p, 1, 16, 1024, 5, 1, 0, p) == arg             # bad scheme
    assert _price(L, p, 1, 16, 1024, 0x2000, 1, 0, p) == arg        # unknown flag
    assert _price(L, p, 1, 16, 1024, _lib.TRAIN_DYNAMIC, 1, 0, p) == arg  # another call's flag
    assert _price(L, p, 1, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg
    assert "SMC_MATH_REF" in _lib.last_error()
    assert _price(L, p, 1, 16, 1024, _lib.MATH_REF | _lib.MATH_HW, 1, 0, p) == arg
    assert _price(L, p, 1, 16, 1024, _lib.MATH_HW, 1, _lib.DTYPE_F64, p) == arg  # f64 has no HW math
    assert "f32 only" in _lib.last_error()
    assert _price(L, p, 1, 16, 1024, 0, 7, 0, p) == arg             # bad normalization
    assert _price(L, p, 1, 0, 1024, 0, 1, 0, p) == shape            # T <= 0
    assert _price(L, p, 1, -3, 1024, 0, 1, 0, p) == shape
    assert _price(L, p, 1, 16, 0, 0, 1, 0, p) == shape              # P <= 0
    assert _price(L, p, 1, 16, -8, 0, 1, 0, p) == shape
    assert _price(L, p, -1, 16, 1024, 0, 1, 0, p) == shape          # B < 0
    # the errors are checked before the empty batch is accepted
    assert _price(L, p, 0, 16, 1024, _lib.MATH_REF, 1, 0, p) == arg


def test_price_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 8)()
    p = ctypes.addressof(dummy)
    for scheme in (0, 1, _lib.MATH_HW, _lib.PRICE_REPLAY):
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            assert _price(L, p, 0, 16, 1024, scheme, norm, 0, p) == _lib.SMC_OK
    assert _price(L, p, 0, 16, 1024, 0, 1, _lib.DTYPE_F64, p) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_price_kernel_choice() -> None:
    L = _lib.lib()

    def name(T, P, scheme, norm, dtype) -> str:
        return L.smc_gbm_price_kernel(T, P, scheme, norm, dtype).decode()

    raw, norm = _lib.NORM_RAW, _lib.NORM_NORMALIZE
    f32, f64 = _lib.DTYPE_F32, _lib.DTYPE_F64
    for dtype in (f32, f64):
        for scheme in (0, 1):
            assert name(16, 4096, scheme, raw, dtype) == "price_kernel(raw)"
            assert name(16, 1 << 20, scheme, raw, dtype) == "price_kernel(raw)"
    assert name(16, 4096, 0, norm, f32) == "price_kernel(lds)"
    assert name(16, 4096, _lib.MATH_HW, norm, f32) == "price_kernel(lds)"
    assert name(3, 693, 1, norm, f32) == "price_kernel(lds)"
    assert name(16, 4096, 0, norm, f64) == "price_kernel(lds)"
    assert name(16, 1 << 20, 0, norm, f32) == "price_kernel(replay)"
    assert name(16, 65536, 0, norm, f32) == "price_kernel(replay)"
    assert name(16, 1 << 20, 0, norm, f64) == "price_kernel(replay)"
    # the flag forces replay at any NORMALIZE shape; RAW has one pass either way
    for P in (1, 528, 4096, 1 << 20):
        assert name(16, P, _lib.PRICE_REPLAY, norm, f32) == "price_kernel(replay)"
        assert name(16, P, 1 | _lib.PRICE_REPLAY | _lib.MATH_HW, norm, f32) == "price_kernel(replay)"
        assert name(16, P, _lib.PRICE_REPLAY, norm, f64) == "price_kernel(replay)"
    assert name(16, 4096, _lib.PRICE_REPLAY, raw, f32) == "price_kernel(raw)"
    # one switch point per element size, and what is parked fits a CU's 160 KiB of LDS beside the 320 B of
    # reduction scratch (f64: and the 51,232 B static table image of the f64 path math)
    for dtype, esz, fixed in ((f32, 4, 320), (f64, 8, 320 + 51232)):
        modes = [name(1, P, 0, norm, dtype) for P in range(1, 1 << 16)]
        edge = max(i for i, m in enumerate(modes) if m == "price_kernel(lds)") + 1
        assert modes[:edge] == ["price_kernel(lds)"] * edge
        assert modes[edge:] == ["price_kernel(replay)"] * (len(modes) - edge)
        assert 64 * 1024 <= edge * esz and edge * esz + fixed <= 160 * 1024, (dtype, edge)
    # shapes and modes the call rejects
    assert name(16, 4096, _lib.MATH_REF, norm, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_REF, raw, f32) == "unsupported"
    assert name(16, 4096, _lib.MATH_HW, norm, f64) == "unsupported"
    assert name(16, 4096, 0, norm, 9) == "unsupported"
    assert name(0, 4096, 0, norm, f32) == "unsupported"
    assert name(16, 0, 0, norm, f32) == "unsupported"
    assert name(16, 4096, 5, norm, f32) == "unsupported"


def test_price_constants_match_the_header() -> None:
    text = open(HEADER).read()

    def define(macro: str) -> int:
        return int(re.search(rf"#define\s+{macro}\s+(\w+)", text).group(1), 0)

    assert _lib.PRICE_COLS == 8 == define("SMC_PRICE_COLS")
    assert _lib.PRICE_REPLAY == 0x800 == define("SMC_PRICE_REPLAY")
    assert _lib.ABI_VERSION == define("SMC_ABI_VERSION") >= 16
    # the flag shares `scheme` with these: no common bit
    others = [_lib.MATH_HW, _lib.MATH_REF, _lib.TRAIN_DYNAMIC, 0xff]
    assert all(_lib.PRICE_REPLAY & o == 0 for o in others)
    assert set(_lib.SIGNATURES) >= {"smc_gbm_price", "smc_gbm_price_kernel"}
    assert len(_lib.SIGNATURES["smc_gbm_price"][1]) == 12 and len(_lib.SIGNATURES["smc_gbm_price_kernel"][1]) == 5
