"""smc_basket_price / smc_basket_price_kernel on the host: argument errors come back as status codes (with a
last_error text that names the argument) before any HIP call and before the empty batch is accepted, the
kernel name follows the flags and the parking bound, the binding's constants match the header, and
basket_price rejects malformed tensors before any device work.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from spectralmc_amd import _lib
from spectralmc_amd.basket import BasketConfig, BasketPrices, basket_price

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
PARK = 144 * 1024


def _call(L, contracts, B, A, T, P, math, norm, out, tsum=None) -> int:
    return int(L.smc_basket_price(contracts, B, A, T, P, 7, None, 0, math, norm, out, tsum, None))


def test_basket_price_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 18)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    for B in (1, 0):  # the errors are checked before the empty batch is accepted
        for tsum in (None, p):
            assert _call(L, None, B, 4, 16, 1024, 0, NORM, p, tsum) == arg
            assert "contracts_dev" in _lib.last_error()
            assert _call(L, p, B, 4, 16, 1024, 0, NORM, None, tsum) == arg
            assert "prices_dev" in _lib.last_error()
            for A in (0, 9, -1, 64):
                assert _call(L, p, B, A, 16, 1024, 0, NORM, p, tsum) == arg, A
                assert "n_assets" in _lib.last_error()
            for norm in (7, -1, 2):
                assert _call(L, p, B, 4, 16, 1024, 0, norm, p, tsum) == arg, norm
                assert "normalization" in _lib.last_error()
            for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | _lib.MATH_HW, 1, 0x2000, -1,
                         _lib.MATH_HW | _lib.PRICE_REPLAY | _lib.TRAIN_DYNAMIC):
                assert _call(L, p, B, 4, 16, 1024, math, NORM, p, tsum) == arg, math
                assert "math" in _lib.last_error()
            for T in (0, -3):
                assert _call(L, p, B, 4, T, 1024, 0, NORM, p, tsum) == shape, T
                assert "timesteps" in _lib.last_error()
            for P in (0, -8, 1 << 40, 1 << 62):  # the engine's limit (gbm.hip validate_common): P < 2^40
                assert _call(L, p, B, 4, 16, P, 0, NORM, p, tsum) == shape, P
                assert "n_paths" in _lib.last_error()
        for bad_b in (-1, 1 << 31, 1 << 40):
            assert _call(L, p, bad_b, 4, 16, 1024, 0, NORM, p) == shape, bad_b
            assert "n_contracts" in _lib.last_error()
    assert all(v == 0.0 for v in dummy)


def test_basket_price_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 18)()
    p = ctypes.addressof(dummy)
    for A in range(1, 9):
        for norm in (RAW, NORM):
            for math in (0, _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.MATH_HW | _lib.PRICE_REPLAY):
                for tsum in (None, p):
                    for T, P in ((16, 1024), (1, 1), (5, 693), (16, (1 << 40) - 1)):
                        assert _call(L, p, 0, A, T, P, math, norm, p, tsum) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_basket_price_kernel_names() -> None:
    L = _lib.lib()

    def name(A, T, P, math, norm) -> str:
        return L.smc_basket_price_kernel(A, T, P, math, norm).decode()

    hw, replay = _lib.MATH_HW, _lib.PRICE_REPLAY
    for A in range(1, 9):
        for math in (0, hw, replay, hw | replay):
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20), (16, (1 << 40) - 1)):
                assert name(A, T, P, math, RAW) == "basket_price_kernel(raw)"
        for math in (replay, hw | replay):
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20)):
                assert name(A, T, P, math, NORM) == "basket_price_kernel(replay)"
        for math in (0, hw):
            assert name(A, 3, 1, math, NORM) == "basket_price_kernel(lds)"
            assert name(A, 3, 693, math, NORM) == "basket_price_kernel(lds)"
    for math in (0, hw):
        assert name(4, 16, 8192, math, NORM) == "basket_price_kernel(lds)"     # 128 KiB parked
        assert name(4, 16, 131072, math, NORM) == "basket_price_kernel(replay)"  # C5: 2 MiB
    # one switch from lds to replay per asset count, at the parking bound
    for A in range(1, 9):
        lo = 128 * 1024 // (4 * A) - 64
        ps = list(range(lo - lo % 4 + 1, PARK // (4 * A) + 64))
        names = [name(A, 16, P, 0, NORM) for P in ps]
        assert names[0] == "basket_price_kernel(lds)" and names[-1] == "basket_price_kernel(replay)"
        edge = names.index("basket_price_kernel(replay)")
        assert names[:edge] == ["basket_price_kernel(lds)"] * edge
        assert names[edge:] == ["basket_price_kernel(replay)"] * (len(names) - edge)
        parked = [A * ((P + 3) // 4 * 4) * 4 for P in ps]
        assert max(parked[:edge]) <= PARK, A
        assert parked[edge] >= 128 * 1024, A
        # below the scanned range everything parks (spot checks), above it everything replays
        assert {name(A, 16, P, 0, NORM) for P in (1, 2, 3, 4, 5, 2047, 2048, 2049, ps[0] - 1)} == {"basket_price_kernel(lds)"}
        assert {name(A, 16, P, 0, NORM) for P in (ps[-1] + 1, 1 << 20, (1 << 40) - 1)} == {"basket_price_kernel(replay)"}
    # flags, asset counts and shapes the call rejects
    for norm in (RAW, NORM):
        for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | hw, 1, 0x2000, -1):
            assert name(4, 16, 4096, math, norm) == "unsupported", math
        for A in (0, 9, -1):
            assert name(A, 16, 4096, 0, norm) == "unsupported", A
        assert name(4, 0, 4096, 0, norm) == "unsupported"
        assert name(4, -1, 4096, 0, norm) == "unsupported"
        assert name(4, 16, 0, 0, norm) == "unsupported"
        assert name(4, 16, -4, 0, norm) == "unsupported"
        assert name(4, 16, 1 << 40, 0, norm) == "unsupported"
    assert name(4, 16, 4096, 0, 7) == "unsupported"
    assert name(4, 16, 4096, 0, -1) == "unsupported"


def test_basket_price_constants_match_the_header() -> None:
    text = open(HEADER).read()

    def define(macro: str) -> int:
        return int(re.search(rf"#define\s+{macro}\s+(\w+)", text).group(1), 0)

    assert _lib.BASKET_PRICE_COLS == 18 == define("SMC_BASKET_PRICE_COLS")
    assert _lib.ABI_VERSION == define("SMC_ABI_VERSION") >= 18
    assert set(_lib.SIGNATURES) >= {"smc_basket_price", "smc_basket_price_kernel"}
    assert len(_lib.SIGNATURES["smc_basket_price"][1]) == 13
    assert len(_lib.SIGNATURES["smc_basket_price_kernel"][1]) == 5
    assert _lib.SIGNATURES["smc_basket_price"][0] is ctypes.c_int32
    assert _lib.SIGNATURES["smc_basket_price_kernel"][0] is ctypes.c_char_p
    # the training call keeps its own shape
    assert len(_lib.SIGNATURES["smc_basket_train_targets"][1]) == 20
    # the dataclass has one field per column, the terminal sums and the block
    fields = list(BasketPrices.__dataclass_fields__)
    assert len(fields) == 18 + 2 and fields[-2:] == ["terminal_sum", "block"]
    assert fields[:6] == ["basket_put", "basket_call", "best_of_put", "best_of_call", "worst_of_put", "worst_of_call"]
    assert fields[6:12] == [f + "_stderr" for f in fields[:6]]
    assert fields[12:18] == ["mean_basket", "mean_best", "mean_worst", "put_exercise_share", "basket_put_intrinsic",
                             "basket_call_intrinsic"]


def test_basket_price_rejects_malformed_tensors_before_device_work() -> None:
    cfg = BasketConfig(n_assets=4, timesteps=16, network_size=64, batches_per_mc_run=32)
    good = torch.zeros((3, cfg.dim), dtype=torch.float64)
    for bad in (good.to(torch.float32), good[:, :cfg.dim - 1], torch.zeros((3, cfg.dim + 1), dtype=torch.float64),
                good.reshape(-1), good.reshape(3, 1, cfg.dim), torch.zeros((3, 2 * cfg.dim), dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match="contracts must be a contiguous"):
            basket_price(bad, cfg)
    for n in (0, -5):
        with pytest.raises(ValueError, match="n_paths"):
            basket_price(good, cfg, n_paths=n)
