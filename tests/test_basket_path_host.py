"""smc_basket_price_paths / smc_basket_price_paths_kernel on the host: argument errors come back as status codes (with
a last_error text that names the argument) in smc_basket_price_general's order, then the scale-table check, all
before any HIP call and before the empty batch is accepted; the kernel name follows the normalisation and math and is
"unsupported" for every rejected call; the binding's constants match the header; basket_price_paths rejects malformed
barriers, weights and correlations before any device work; validate=True's new checks, run on CPU tensors.  CPU only
(no kernel launches)."""

from __future__ import annotations

import ctypes
import inspect
import os
import re

import pytest
import torch

from spectralmc_amd import _lib, basket
from spectralmc_amd.basket import (BASKET_PATH_FIELDS, BasketConfig, BasketEngine, BasketPathPrices,
                                   basket_price_paths, validate_basket_barriers)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
LDS = 144 * 1024
SCRATCH = 2112  # bytes of scratch at the head of the dynamic LDS (the header states it)
ROW = 512 * 8   # one row of per-lane f64 accumulators


def _fits(A: int, T: int) -> bool:
    """The header's rule: the scratch, the A T f32 scales (padded to 8 bytes) and one date of accumulators."""
    return SCRATCH + (A * T * 4 + 7) // 8 * 8 + A * ROW <= LDS


def _call(L, contracts, B, A, T, P, math, norm, out, tsum=None, w=None, ws=0, c=None, cs=0, bars=None) -> int:
    return int(L.smc_basket_price_paths(contracts, w, ws, c, cs, bars, B, A, T, P, 7, None, 0, math, norm, out, tsum,
                                        None))


def test_path_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 25)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    for B in (1, 0):  # the errors are checked before the empty batch is accepted
        for tsum, bars in ((None, None), (p, p)):
            for w, c in ((None, None), (p, p)):
                kw = dict(w=w, ws=4, c=c, cs=6, bars=bars)
                assert _call(L, None, B, 4, 16, 1024, 0, NORM, p, tsum, **kw) == arg
                assert "smc_basket_price_paths" in _lib.last_error() and "contracts_dev" in _lib.last_error()
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, None, tsum, **kw) == arg
                assert "prices_dev" in _lib.last_error()
                for A in (0, 9, -1, 64):
                    assert _call(L, p, B, A, 16, 1024, 0, NORM, p, tsum, **kw) == arg, A
                    assert "n_assets" in _lib.last_error()
                for norm in (7, -1, 2):
                    assert _call(L, p, B, 4, 16, 1024, 0, norm, p, tsum, **kw) == arg, norm
                    assert "normalization" in _lib.last_error()
                for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | _lib.MATH_HW, 1, 0x2000, -1,
                             _lib.MATH_HW | _lib.PRICE_REPLAY | _lib.TRAIN_DYNAMIC):
                    assert _call(L, p, B, 4, 16, 1024, math, NORM, p, tsum, **kw) == arg, math
                    assert "math" in _lib.last_error()
                for T in (0, -3):
                    assert _call(L, p, B, 4, T, 1024, 0, NORM, p, tsum, **kw) == shape, T
                    assert "timesteps" in _lib.last_error()
                for P in (0, -8, 1 << 40, 1 << 62):
                    assert _call(L, p, B, 4, 16, P, 0, NORM, p, tsum, **kw) == shape, P
                    assert "n_paths" in _lib.last_error()
            for ws in (1, 3, -1, -4):
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, tsum, w=p, ws=ws, bars=bars) == arg, ws
                assert "weights_stride" in _lib.last_error()
            for cs in (1, 5, -1, -6):
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, tsum, c=p, cs=cs, bars=bars) == arg, cs
                assert "corr_stride" in _lib.last_error()
            # the order: the price call's checks, the weights' stride, the correlation's, then the scale table
            big = 40000  # 4 * 40000 scales are 640000 bytes
            assert _call(L, p, B, 4, big, 1024, 0, NORM, p, tsum, w=p, ws=3, c=p, cs=5, bars=bars) == arg
            assert "weights_stride" in _lib.last_error()
            assert _call(L, p, B, 4, big, 1024, 0, NORM, p, tsum, c=p, cs=5, bars=bars) == arg
            assert "corr_stride" in _lib.last_error()
            assert _call(L, p, B, 4, big, 1024, 0, NORM, p, tsum, w=p, ws=4, c=p, cs=6, bars=bars) == shape
            assert "scales" in _lib.last_error() and "timesteps" in _lib.last_error()
            assert _call(L, p, B, 4, big, 0, 0, NORM, p, tsum, bars=bars) == shape
            assert "n_paths" in _lib.last_error()
            assert _call(L, p, B, 9, big, 1024, 0, NORM, p, tsum, w=p, ws=3, bars=bars) == arg
            assert "n_assets" in _lib.last_error()
            assert _call(L, p, B, 4, 0, 1024, 0, NORM, p, tsum, w=p, ws=3, c=p, cs=5, bars=bars) == shape
            assert "timesteps" in _lib.last_error()
        for bad_b in (-1, 1 << 31, 1 << 40):
            assert _call(L, p, bad_b, 4, 16, 1024, 0, NORM, p) == shape, bad_b
            assert "n_contracts" in _lib.last_error()
    assert all(v == 0.0 for v in dummy)


def test_path_scale_table_bound() -> None:
    """NORMALIZE is rejected exactly where the header's rule says the table does not fit; RAW has no table."""
    L = _lib.lib()
    dummy = (ctypes.c_double * 25)()
    p = ctypes.addressof(dummy)
    for A in range(1, 9):
        edge = max(T for T in range(1, LDS // (4 * A) + 2) if _fits(A, T))
        assert edge > 1000
        for T in (1, 16, 40, edge - 1, edge):
            assert _fits(A, T)
            for math in (0, _lib.MATH_HW):
                assert _call(L, p, 0, A, T, 693, math, NORM, p) == _lib.SMC_OK, (A, T)
                assert L.smc_basket_price_paths_kernel(A, T, 693, math, NORM) == b"basket_path_kernel(replay)"
        for T in (edge + 1, edge + 2, 2 * edge, (1 << 31) - 1):
            assert not _fits(A, T)
            for B in (0, 1):
                assert _call(L, p, B, A, T, 693, 0, NORM, p) == _lib.SMC_ERR_INVALID_SHAPE, (A, T)
                assert "scales" in _lib.last_error()
            assert L.smc_basket_price_paths_kernel(A, T, 693, 0, NORM) == b"unsupported"
            assert _call(L, p, 0, A, T, 693, 0, RAW, p) == _lib.SMC_OK
            assert L.smc_basket_price_paths_kernel(A, T, 693, 0, RAW) == b"basket_path_kernel(raw)"
    assert all(v == 0.0 for v in dummy)


def test_path_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 25)()
    p = ctypes.addressof(dummy)
    for A in range(1, 9):
        n = A * (A - 1) // 2
        for norm in (RAW, NORM):
            for math in (0, _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.MATH_HW | _lib.PRICE_REPLAY):
                for tsum, bars in ((None, None), (p, p), (None, p)):
                    for T, P in ((16, 1024), (1, 1), (5, 693), (16, (1 << 40) - 1)):
                        assert _call(L, p, 0, A, T, P, math, norm, p, tsum, bars=bars) == _lib.SMC_OK
                        for ws, cs in ((0, 0), (A, n), (A + 3, n + 5)):
                            assert _call(L, p, 0, A, T, P, math, norm, p, tsum, w=p, ws=ws, c=p, cs=cs,
                                         bars=bars) == _lib.SMC_OK
                        assert _call(L, p, 0, A, T, P, math, norm, p, tsum, ws=-7, cs=-7, bars=bars) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_path_kernel_names() -> None:
    L = _lib.lib()

    def name(A, T, P, math, norm) -> str:
        return L.smc_basket_price_paths_kernel(A, T, P, math, norm).decode()

    hw, replay = _lib.MATH_HW, _lib.PRICE_REPLAY
    for A in range(1, 9):
        for math in (0, hw, replay, hw | replay):  # SMC_PRICE_REPLAY is accepted and changes nothing
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20), (16, (1 << 40) - 1), (16, 131072)):
                assert name(A, T, P, math, RAW) == "basket_path_kernel(raw)"
                assert name(A, T, P, math, NORM) == "basket_path_kernel(replay)"
    for norm in (RAW, NORM):
        for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | hw, 1, 0x2000, -1):
            assert name(4, 16, 4096, math, norm) == "unsupported", math
        for A in (0, 9, -1):
            assert name(A, 16, 4096, 0, norm) == "unsupported", A
        for T, P in ((0, 4096), (-1, 4096), (16, 0), (16, -4), (16, 1 << 40)):
            assert name(4, T, P, 0, norm) == "unsupported"
    assert name(4, 16, 4096, 0, 7) == "unsupported"
    assert name(4, 16, 4096, 0, -1) == "unsupported"
    assert name(8, 4000, 2048, 0, NORM) == "unsupported" and name(8, 4000, 2048, 0, RAW) == "basket_path_kernel(raw)"


def test_path_constants_match_the_header() -> None:
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+SMC_ABI_VERSION\s+(\w+)", text).group(1))
    assert "smc_basket_price_paths" in re.search(r"#define\s+SMC_ABI_VERSION.*", text).group(0)
    assert _lib.BASKET_PATH_COLS == 25 == int(re.search(r"#define\s+SMC_BASKET_PATH_COLS\s+(\d+)", text).group(1))
    sig = _lib.SIGNATURES["smc_basket_price_paths"]
    assert sig[0] is ctypes.c_int32 and len(sig[1]) == 18
    # smc_basket_price_general's arguments with the barriers after the correlation's stride
    general = _lib.SIGNATURES["smc_basket_price_general"][1]
    assert sig[1][:5] + sig[1][6:] == general and sig[1][5] is ctypes.c_void_p
    assert _lib.SIGNATURES["smc_basket_price_paths_kernel"] == _lib.SIGNATURES["smc_basket_price_general_kernel"]
    decl = re.search(r"int32_t smc_basket_price_paths\((.*?)\);", text, flags=re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 18
    section = text[text.index("path-dependent basket pricing"):]
    assert f"{SCRATCH}\n * bytes of scratch" in section or f"{SCRATCH} bytes of scratch" in section
    assert "no path-dependent basket payoffs" not in text
    # the Python surface
    assert len(BASKET_PATH_FIELDS) == 25 == len(set(BASKET_PATH_FIELDS))
    fields = [f.name for f in BasketPathPrices.__dataclass_fields__.values()]
    assert fields == list(BASKET_PATH_FIELDS) + ["terminal_sum", "block"]
    assert BasketPathPrices.__dataclass_params__.frozen
    for k in range(10):
        assert BASKET_PATH_FIELDS[10 + k] == BASKET_PATH_FIELDS[k] + "_stderr"
    params = inspect.signature(basket_price_paths).parameters
    assert list(params) == ["contracts", "cfg", "barriers", "weights", "correlation", "ordinal0", "n_paths", "validate"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[2:])
    assert [params[k].default for k in list(params)[2:]] == [None, None, None, 0, None, False]
    eng = inspect.signature(BasketEngine.price_paths).parameters
    assert all(eng[k].default == params[k].default for k in list(params)[2:])
    for name in ("BASKET_PATH_FIELDS", "BasketPathPrices", "basket_price_paths"):
        assert name in basket.__all__


def test_basket_price_paths_rejects_malformed_inputs_before_device_work() -> None:
    A, B = 4, 3
    cfg = BasketConfig(n_assets=A, timesteps=16, network_size=64, batches_per_mc_run=32)
    good = torch.zeros((B, cfg.dim), dtype=torch.float64)
    bars = torch.tensor([[50.0, 150.0, 20.0]] * B, dtype=torch.float64)
    for bad in (bars.to(torch.float32), bars[:, :2], bars[:2], bars.reshape(-1), bars[0].contiguous(),
                torch.zeros((B, 6), dtype=torch.float64)[:, ::2], torch.zeros((B, 4), dtype=torch.float64),
                bars.numpy(), [[50.0, 150.0, 20.0]] * B):
        with pytest.raises(ValueError, match="barriers must be a contiguous float64 tensor of shape"):
            basket_price_paths(good, cfg, barriers=bad)
    w = torch.full((B, A), 0.25, dtype=torch.float64)
    for bad in (w.to(torch.float32), w[:, :3], torch.zeros((B + 1, A), dtype=torch.float64), w.reshape(-1), w.numpy()):
        with pytest.raises(ValueError, match="weights must be a contiguous float64"):
            basket_price_paths(good, cfg, weights=bad, barriers=bars)
    C = torch.eye(A, dtype=torch.float64)
    for bad in (C.to(torch.float32), C[:3], torch.zeros((B + 1, A, A), dtype=torch.float64),
                torch.zeros(5, dtype=torch.float64), C.numpy()):
        with pytest.raises(ValueError, match="correlation must be a contiguous float64"):
            basket_price_paths(good, cfg, correlation=bad)
    # well-formed tensors in host memory: named before the device is asked for, the barriers first
    with pytest.raises(ValueError, match="barriers must be a device tensor"):
        basket_price_paths(good, cfg, barriers=bars, weights=w, correlation=C)
    with pytest.raises(ValueError, match="weights must be a device tensor"):
        basket_price_paths(good, cfg, weights=w, correlation=C)
    with pytest.raises(ValueError, match="correlation must be a device tensor"):
        basket_price_paths(good, cfg, correlation=C)
    with pytest.raises(ValueError, match="contracts must be a contiguous"):
        basket_price_paths(good.to(torch.float32), cfg, barriers=bars[:, :2])
    with pytest.raises(ValueError, match="n_paths must be positive"):
        basket_price_paths(good, cfg, n_paths=0)


def test_validate_barriers_on_cpu_tensors() -> None:
    inf = float("inf")
    ok = torch.tensor([[50.0, 150.0, 20.0], [-inf, inf, -inf], [-3.0, 2.0, 1.0], [-inf, 0.0, inf], [0.0, 1e-300, 5.0]],
                      dtype=torch.float64)
    validate_basket_barriers(ok)
    validate_basket_barriers(None)
    for col in range(3):
        bad = ok.clone()
        bad[2, col] = float("nan")
        with pytest.raises(ValueError, match="NaN"):
            validate_basket_barriers(bad)
    for lo, up in ((150.0, 50.0), (1.0, 1.0), (inf, inf), (-inf, -inf), (0.0, -0.0)):
        bad = ok.clone()
        bad[3, 0], bad[3, 1] = lo, up
        with pytest.raises(ValueError, match="lower < upper"):
            validate_basket_barriers(bad)
