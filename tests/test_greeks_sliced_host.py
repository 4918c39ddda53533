"""smc_gbm_greeks_sliced and its two queries on the host: every rejection comes back as its status code before any HIP
call and in the documented order (smc_gbm_greeks' checks, then the forcing flags, then smc_gbm_price_sliced's slice,
grid and workspace checks), the empty batch is accepted only after the checks, the kernel name and the workspace size
follow their formulas, and the binding matches the header.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import os
import re

from spectralmc_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
ARG, SHAPE = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
F32, F64 = _lib.DTYPE_F32, _lib.DTYPE_F64
LOG, SIMPLE = 0, 1
BIG = 1 << 40  # a workspace size no check objects to


def _sliced(L, contracts, B, T, P, span, scheme, norm, dtype, out, ws, ws_bytes) -> int:
    return int(L.smc_gbm_greeks_sliced(contracts, B, T, P, span, 7, None, 0, scheme, norm, dtype, out, ws, ws_bytes,
                                       None))


def _bytes(B: int, P: int, span: int) -> int:
    return int(_lib.lib().smc_gbm_greeks_sliced_workspace_bytes(B, P, span))


def test_greeks_sliced_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 26)()
    p = ctypes.addressof(dummy)

    def call(contracts=p, B=1, T=16, P=4096, span=2048, scheme=LOG, norm=NORM, dtype=F32, out=p, ws=p, nbytes=BIG):
        return _sliced(L, contracts, B, T, P, span, scheme, norm, dtype, out, ws, nbytes)

    # 1. smc_gbm_greeks' checks, under the new name
    assert call(contracts=None) == ARG
    assert "contracts" in _lib.last_error()
    assert call(T=0) == SHAPE and call(T=-3) == SHAPE
    assert call(P=0) == SHAPE and call(P=-8) == SHAPE and call(P=1 << 40) == SHAPE
    assert call(B=-1) == SHAPE and call(B=1 << 31) == SHAPE
    assert call(dtype=9) == ARG
    assert call(out=None) == ARG
    assert "smc_gbm_greeks_sliced: greeks_dev" in _lib.last_error()
    assert call(scheme=5) == ARG
    assert "smc_gbm_greeks_sliced: bad scheme" in _lib.last_error()
    assert call(scheme=0x2000) == ARG
    assert "bad scheme" in _lib.last_error()
    assert call(scheme=_lib.MATH_REF) == ARG
    assert "smc_gbm_greeks_sliced: SMC_MATH_REF" in _lib.last_error()
    assert call(scheme=_lib.MATH_REF | _lib.MATH_HW) == ARG
    assert call(scheme=_lib.MATH_HW, dtype=F64) == ARG
    assert "smc_gbm_greeks_sliced: SMC_MATH_HW is f32 only" in _lib.last_error()
    assert call(norm=7) == ARG
    assert "smc_gbm_greeks_sliced: bad normalization" in _lib.last_error()
    for scheme in (SIMPLE, SIMPLE | _lib.MATH_HW):
        assert call(scheme=scheme) == ARG
        assert "smc_gbm_greeks_sliced: SMC_SCHEME_SIMPLE_EULER is not supported" in _lib.last_error()
    # 2. there is no mode to force
    for flag in (_lib.PRICE_REPLAY, _lib.TRAIN_DYNAMIC, _lib.PRICE_REPLAY | _lib.MATH_HW):
        assert call(scheme=flag) == ARG
        assert "no mode to force" in _lib.last_error()
    # 3. the slice length
    for span in (0, -2048, 1, 2047, 2049, 1024, 4096 + 512):
        assert call(span=span) == SHAPE, span
        assert "multiple of 2048" in _lib.last_error()
    # 4. the grid: W <= 65,535 and B W < 2^31
    assert call(P=65535 * 2048 + 1, span=2048) == SHAPE
    assert "65,535 slices" in _lib.last_error()
    assert call(B=1 << 16, P=32768 * 2048, span=2048) == SHAPE   # B W = 2^31
    assert call(B=(1 << 16) + 1, P=32768 * 2048, span=2048) == SHAPE
    # 5. the workspace
    assert call(ws=None) == ARG
    assert "workspace_dev is NULL" in _lib.last_error()
    need = _bytes(1, 4096, 2048)
    assert need == 8 * (22 * 2 + 2)
    assert call(nbytes=need - 1) == ARG
    assert "workspace_bytes" in _lib.last_error()
    assert call(nbytes=0) == ARG and call(nbytes=-1) == ARG
    assert all(v == 0.0 for v in dummy)


def test_greeks_sliced_checks_run_in_order() -> None:
    """A call that breaks two rules reports the earlier one (status and message), all before the empty batch."""
    L = _lib.lib()
    dummy = (ctypes.c_double * 26)()
    p = ctypes.addressof(dummy)
    for B in (1, 0):
        # smc_gbm_greeks' own order: shape before the NULL output, the output before the scheme, SMC_MATH_REF before
        # the normalization, the normalization before simple Euler
        assert _sliced(L, p, B, 0, 4096, 2048, LOG, NORM, F32, None, p, BIG) == SHAPE
        assert _sliced(L, p, B, 16, 4096, 2048, 5, NORM, F32, None, p, BIG) == ARG
        assert "greeks_dev" in _lib.last_error()
        assert _sliced(L, p, B, 16, 4096, 2048, _lib.MATH_REF, 7, F32, p, p, BIG) == ARG
        assert "SMC_MATH_REF" in _lib.last_error()
        assert _sliced(L, p, B, 16, 4096, 2048, SIMPLE, 7, F32, p, p, BIG) == ARG
        assert "bad normalization" in _lib.last_error()
        # simple Euler is the last of smc_gbm_greeks' checks: before a forcing flag
        assert _sliced(L, p, B, 16, 4096, 2048, SIMPLE | _lib.PRICE_REPLAY, NORM, F32, p, p, BIG) == ARG
        assert "SMC_SCHEME_SIMPLE_EULER" in _lib.last_error()
        # a forcing flag with a bad normalization: the normalization is smc_gbm_greeks' check, the flag comes after
        assert _sliced(L, p, B, 16, 4096, 2048, _lib.PRICE_REPLAY, 7, F32, p, p, BIG) == ARG
        assert "bad normalization" in _lib.last_error()
        # a forcing flag before a bad slice length; a bad slice length before a missing workspace
        assert _sliced(L, p, B, 16, 4096, 100, _lib.TRAIN_DYNAMIC, NORM, F32, p, p, BIG) == ARG
        assert "no mode to force" in _lib.last_error()
        assert _sliced(L, p, B, 16, 4096, 100, LOG, NORM, F32, p, None, 0) == SHAPE
        assert "multiple of 2048" in _lib.last_error()
        # too many slices before a missing workspace
        assert _sliced(L, p, B, 16, 65536 * 2048, 2048, LOG, NORM, F32, p, None, 0) == SHAPE
        assert "65,535 slices" in _lib.last_error()
    # the empty batch still needs a workspace pointer, and every other check
    assert _sliced(L, p, 0, 16, 4096, 2048, LOG, NORM, F32, p, None, 0) == ARG
    assert _sliced(L, p, 0, 16, 4096, 2048, _lib.MATH_REF, NORM, F32, p, p, 0) == ARG
    assert _sliced(L, p, 0, 16, 4096, 2048, _lib.PRICE_REPLAY, NORM, F32, p, p, 0) == ARG
    assert _sliced(L, p, 0, 16, 4096, 2048, SIMPLE, NORM, F32, p, p, 0) == ARG
    assert _sliced(L, p, 0, 16, 4096, 2047, LOG, NORM, F32, p, p, 0) == SHAPE
    assert all(v == 0.0 for v in dummy)


def test_greeks_sliced_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 26)()
    p = ctypes.addressof(dummy)
    assert _bytes(0, 4096, 2048) == 0
    for scheme in (LOG, LOG | _lib.MATH_HW):
        for norm in (RAW, NORM):
            for P, span in ((4096, 2048), (693, 2048), (1 << 24, 32768)):
                assert _sliced(L, p, 0, 16, P, span, scheme, norm, F32, p, p, 0) == _lib.SMC_OK
    assert _sliced(L, p, 0, 16, 4096, 2048, LOG, NORM, F64, p, p, 0) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_greeks_sliced_kernel_name() -> None:
    L = _lib.lib()

    def name(T=16, P=4096, span=2048, scheme=LOG, norm=NORM, dtype=F32) -> str:
        return L.smc_gbm_greeks_sliced_kernel(T, P, span, scheme, norm, dtype).decode()

    for dtype in (F32, F64):
        for P, span in ((4096, 2048), (693, 2048), (1, 2048), (1 << 24, 32768), (4096, 1 << 20)):
            assert name(P=P, span=span, norm=RAW, dtype=dtype) == "greeks_slice_kernel(raw)"
            assert name(P=P, span=span, norm=NORM, dtype=dtype) == "greeks_slice_kernel(replay)"
    assert name(scheme=_lib.MATH_HW, norm=RAW) == "greeks_slice_kernel(raw)"
    assert name(scheme=_lib.MATH_HW) == "greeks_slice_kernel(replay)"
    assert name(P=65535 * 2048) == "greeks_slice_kernel(replay)"
    # every combination the call rejects
    rejected = [dict(T=0), dict(T=-1), dict(P=0), dict(P=-5), dict(P=1 << 40), dict(span=0), dict(span=-2048),
                dict(span=2047), dict(span=1024), dict(P=65535 * 2048 + 1), dict(scheme=5), dict(scheme=0x2000),
                dict(scheme=SIMPLE), dict(scheme=SIMPLE | _lib.MATH_HW), dict(scheme=SIMPLE, dtype=F64),
                dict(scheme=_lib.MATH_REF), dict(scheme=_lib.MATH_REF | _lib.MATH_HW),
                dict(scheme=_lib.MATH_HW, dtype=F64), dict(scheme=_lib.PRICE_REPLAY), dict(scheme=_lib.TRAIN_DYNAMIC),
                dict(scheme=_lib.PRICE_REPLAY | _lib.MATH_HW), dict(norm=7), dict(norm=-1), dict(dtype=9)]
    for kw in rejected:
        for norm in (RAW, NORM):
            assert name(**{"norm": norm, **kw}) == "unsupported", kw


def test_greeks_sliced_workspace_bytes() -> None:
    price = _lib.lib().smc_gbm_price_sliced_workspace_bytes
    for B in (0, 1, 14, 4096):
        for P, span in ((1, 2048), (693, 2048), (2048, 2048), (2049, 2048), (6837, 2048), (10241, 4096),
                        (1 << 24, 32768), (65535 * 2048, 2048)):
            W = -(-P // span)
            assert _bytes(B, P, span) == 8 * B * (22 * W + 2), (B, P, span)
    assert _bytes((1 << 31) - 1, 4096, 4096) == 8 * ((1 << 31) - 1) * 24
    # what the price query rejects
    for B, P, span in ((-1, 4096, 2048), (1 << 31, 4096, 4096), (1, 0, 2048), (1, -4, 2048), (1, 1 << 40, 1 << 30),
                       (1, 4096, 0), (1, 4096, -2048), (1, 4096, 2047), (1, 4096, 1000), (1, 65535 * 2048 + 1, 2048),
                       (1 << 16, 32768 * 2048, 2048), (1 << 30, 4096, 2048)):
        assert int(price(B, P, span)) == -1 and _bytes(B, P, span) == -1, (B, P, span)
    assert _bytes((1 << 30) - 1, 4096, 2048) == 8 * ((1 << 30) - 1) * 46  # B W = 2^31 - 2
    # the default slice is the price call's rule: at most 512 slices
    for P in (1, 65536, 1 << 20, (1 << 20) + 1, 1 << 24):
        span = int(_lib.lib().smc_gbm_price_slice_paths(P))
        assert _bytes(1, P, span) == 8 * (22 * -(-P // span) + 2) and -(-P // span) <= 512


def test_greeks_sliced_binding_matches_the_header() -> None:
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == int(re.search(r"#define\s+SMC_ABI_VERSION\s+(\d+)", text).group(1)) == 21
    assert int(_lib.lib().smc_abi_version()) == 21
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn, nargs in (("smc_gbm_greeks_sliced", 15), ("smc_gbm_greeks_sliced_workspace_bytes", 3),
                      ("smc_gbm_greeks_sliced_kernel", 6)):
        decl = re.search(rf"\b{fn}\s*\(([^)]*)\)\s*;", code)
        assert decl, fn
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[fn][1]), fn
    # the new declarations come after the sliced price call's, in the issue's order
    at = [text.index(s) for s in ("const char* smc_gbm_price_sliced_kernel(", "int32_t smc_gbm_greeks_sliced(",
                                  "smc_gbm_greeks_sliced_workspace_bytes(int64_t", "const char* smc_gbm_greeks_sliced_kernel(")]
    assert at == sorted(at)
    restypes = {"smc_gbm_greeks_sliced": ctypes.c_int32, "smc_gbm_greeks_sliced_workspace_bytes": ctypes.c_int64,
                "smc_gbm_greeks_sliced_kernel": ctypes.c_char_p}
    for fn, rt in restypes.items():
        assert _lib.SIGNATURES[fn][0] is rt, fn
    # the same argument types as the sliced price call, whose geometry it takes
    for fn in restypes:
        assert _lib.SIGNATURES[fn][1] == _lib.SIGNATURES[fn.replace("greeks", "price")][1], fn
    # the sliced pricing comment no longer lists sliced Greeks as out of scope
    pricing = text[text.index("---- sliced batched pricing"):text.index("int32_t smc_gbm_price_sliced(")]
    scope = pricing[pricing.index("Out of scope:"):]
    assert "Greeks" not in scope.replace("smc_gbm_greeks_sliced", "") and "path-dependent or basket pricing" in scope
