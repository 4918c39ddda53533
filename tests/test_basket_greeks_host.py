"""smc_basket_greeks / smc_basket_greeks_kernel / smc_basket_greeks_cols on the host: argument errors come back as
status codes (with a last_error text that names the argument) in smc_basket_price's order, before any HIP call and
before the empty batch is accepted; the kernel name follows the flags and the parking bound; the binding's constants
match the header; the dataclass fields follow the column table; and basket_greeks rejects malformed tensors before any
device work.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from spectralmc_amd import _lib
from spectralmc_amd.basket import BasketConfig, BasketEngine, BasketGreeks, _greeks_views, basket_greeks, basket_greeks_fields

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
PARK = 144 * 1024
SCRATCH = 6848  # bytes of LDS the kernel keeps beside the parked block (the header's figure)
NAME = "basket_greeks_kernel"


def _call(L, contracts, B, A, T, P, math, norm, out, sums=None) -> int:
    return int(L.smc_basket_greeks(contracts, B, A, T, P, 7, None, 0, math, norm, out, sums, None))


def test_basket_greeks_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 80)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    for B in (1, 0):  # the errors are checked before the empty batch is accepted
        for sums in (None, p):
            assert _call(L, None, B, 4, 16, 1024, 0, NORM, p, sums) == arg
            assert "contracts_dev" in _lib.last_error()
            assert _call(L, p, B, 4, 16, 1024, 0, NORM, None, sums) == arg
            assert "greeks_dev" in _lib.last_error()
            for A in (0, 9, -1, 64):
                assert _call(L, p, B, A, 16, 1024, 0, NORM, p, sums) == arg, A
                assert "n_assets" in _lib.last_error()
            for norm in (7, -1, 2):
                assert _call(L, p, B, 4, 16, 1024, 0, norm, p, sums) == arg, norm
                assert "normalization" in _lib.last_error()
            for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | _lib.MATH_HW, 1, 0x2000, -1,
                         _lib.MATH_HW | _lib.PRICE_REPLAY | _lib.TRAIN_DYNAMIC):
                assert _call(L, p, B, 4, 16, 1024, math, NORM, p, sums) == arg, math
                assert "math" in _lib.last_error()
            for T in (0, -3):
                assert _call(L, p, B, 4, T, 1024, 0, NORM, p, sums) == shape, T
                assert "timesteps" in _lib.last_error()
            for P in (0, -8, 1 << 40, 1 << 62):
                assert _call(L, p, B, 4, 16, P, 0, NORM, p, sums) == shape, P
                assert "n_paths" in _lib.last_error()
        for bad_b in (-1, 1 << 31, 1 << 40):
            assert _call(L, p, bad_b, 4, 16, 1024, 0, NORM, p) == shape, bad_b
            assert "n_contracts" in _lib.last_error()
    assert all(v == 0.0 for v in dummy)


def test_basket_greeks_argument_errors_come_in_the_price_calls_order() -> None:
    """Every argument wrong at once, then mended one by one in the order of the checks: contracts_dev, greeks_dev,
    n_assets, math, normalization, the shape (n_contracts, timesteps, n_paths), n_paths >= 2^40.  smc_basket_price
    names the same argument at every stage."""
    L = _lib.lib()
    dummy = (ctypes.c_double * 80)()
    p = ctypes.addressof(dummy)
    bad = dict(contracts=None, out=None, A=0, math=1, norm=7, B=-1, T=0, P=1 << 40)
    good = dict(contracts=p, out=p, A=4, math=0, norm=NORM, B=0, T=16, P=1024)
    stages = [("contracts", "contracts_dev"), ("out", "_dev is NULL"), ("A", "n_assets"), ("math", "bad math"),
              ("norm", "normalization"), ("B", "n_contracts"), ("T", "timesteps"), ("P", "n_paths too large")]
    args = dict(bad)
    for key, text in stages:
        for fn in (L.smc_basket_greeks, L.smc_basket_price):
            st = int(fn(args["contracts"], args["B"], args["A"], args["T"], args["P"], 7, None, 0, args["math"], args["norm"],
                        args["out"], None, None))
            assert st != _lib.SMC_OK and text in _lib.last_error(), (key, fn.__name__, _lib.last_error())
        args[key] = good[key]
    assert _call(L, p, 0, 4, 16, 1024, 0, NORM, p) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_basket_greeks_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 80)()
    p = ctypes.addressof(dummy)
    for A in range(1, 9):
        for norm in (RAW, NORM):
            for math in (0, _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.MATH_HW | _lib.PRICE_REPLAY):
                for sums in (None, p):
                    for T, P in ((16, 1024), (1, 1), (5, 693), (16, (1 << 40) - 1)):
                        assert _call(L, p, 0, A, T, P, math, norm, p, sums) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_basket_greeks_kernel_names() -> None:
    L = _lib.lib()

    def name(A, T, P, math, norm) -> str:
        return L.smc_basket_greeks_kernel(A, T, P, math, norm).decode()

    hw, replay = _lib.MATH_HW, _lib.PRICE_REPLAY
    for A in range(1, 9):
        for math in (0, hw, replay, hw | replay):
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20), (16, (1 << 40) - 1)):
                assert name(A, T, P, math, RAW) == f"{NAME}(raw)"
        for math in (replay, hw | replay):
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20)):
                assert name(A, T, P, math, NORM) == f"{NAME}(replay)"
        for math in (0, hw):
            assert name(A, 3, 1, math, NORM) == f"{NAME}(lds)"
            assert name(A, 3, 693, math, NORM) == f"{NAME}(lds)"
    for math in (0, hw):
        assert name(4, 16, 8192, math, NORM) == f"{NAME}(lds)"       # 128 KiB parked
        assert name(4, 16, 131072, math, NORM) == f"{NAME}(replay)"  # C5: 2 MiB
    # one switch from lds to replay per asset count, exactly where the parked block and the scratch pass 144 KiB
    for A in range(1, 9):
        lo = 128 * 1024 // (4 * A) - 64
        ps = list(range(lo - lo % 4 + 1, PARK // (4 * A) + 64))
        names = [name(A, 16, P, 0, NORM) for P in ps]
        assert names[0] == f"{NAME}(lds)" and names[-1] == f"{NAME}(replay)"
        edge = names.index(f"{NAME}(replay)")
        assert names[:edge] == [f"{NAME}(lds)"] * edge
        assert names[edge:] == [f"{NAME}(replay)"] * (len(names) - edge)
        parked = [A * ((P + 3) // 4 * 4) * 4 + SCRATCH for P in ps]
        assert max(parked[:edge]) <= PARK < parked[edge], A
        assert {name(A, 16, P, 0, NORM) for P in (1, 2, 3, 4, 5, 2047, 2048, 2049, ps[0] - 1)} == {f"{NAME}(lds)"}
        assert {name(A, 16, P, 0, NORM) for P in (ps[-1] + 1, 1 << 20, (1 << 40) - 1)} == {f"{NAME}(replay)"}
    # flags, asset counts and shapes the call rejects
    for norm in (RAW, NORM):
        for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | hw, 1, 0x2000, -1):
            assert name(4, 16, 4096, math, norm) == "unsupported", math
        for A in (0, 9, -1):
            assert name(A, 16, 4096, 0, norm) == "unsupported", A
        for T, P in ((0, 4096), (-1, 4096), (16, 0), (16, -4), (16, 1 << 40)):
            assert name(4, T, P, 0, norm) == "unsupported"
    assert name(4, 16, 4096, 0, 7) == "unsupported"
    assert name(4, 16, 4096, 0, -1) == "unsupported"


def test_basket_greeks_cols() -> None:
    L = _lib.lib()
    for A in range(1, 9):
        assert L.smc_basket_greeks_cols(A) == 8 * A + 16 == _lib.basket_greeks_cols(A) == len(basket_greeks_fields(A))
    for A in (0, 9, -1, 64):
        assert L.smc_basket_greeks_cols(A) == -1
        with pytest.raises(ValueError, match="n_assets"):
            _lib.basket_greeks_cols(A)
        with pytest.raises(ValueError, match="n_assets"):
            basket_greeks_fields(A)


def test_basket_greeks_constants_match_the_header() -> None:
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == int(re.search(r"#define\s+SMC_ABI_VERSION\s+(\w+)", text).group(1)) >= 20
    assert _lib.lib().smc_abi_version() == _lib.ABI_VERSION
    for symbol in ("smc_basket_greeks", "smc_basket_greeks_kernel", "smc_basket_greeks_cols"):
        assert symbol in _lib.SIGNATURES and re.search(rf"\b{symbol}\(", text), symbol
    assert len(_lib.SIGNATURES["smc_basket_greeks"][1]) == 13 == len(_lib.SIGNATURES["smc_basket_price"][1])
    assert _lib.SIGNATURES["smc_basket_greeks"][1] == _lib.SIGNATURES["smc_basket_price"][1]
    assert _lib.SIGNATURES["smc_basket_greeks_kernel"] == _lib.SIGNATURES["smc_basket_price_kernel"]
    assert _lib.SIGNATURES["smc_basket_greeks_cols"] == (ctypes.c_int32, [ctypes.c_int32])
    # the parking bound the name test checks is the documented one
    assert re.search(rf"{SCRATCH}\s+(\*\s+)?bytes of scratch fit in 144 KiB", text)


def test_basket_greeks_fields_follow_the_column_table() -> None:
    fields = list(BasketGreeks.__dataclass_fields__)
    kinds = ["delta", "vega", "rho", "theta", "correlation"]
    means = [f"{k}_{side}" for k in kinds for side in ("put", "call")]
    assert fields == means + [m + "_stderr" for m in means] + ["put", "call", "put_stderr", "call_stderr", "terminal_sum",
                                                               "sum_xl", "sum_xc", "block"]
    for A in (1, 3, 8):
        n, B = 4 * A + 6, 5
        block = torch.arange(B * (8 * A + 16), dtype=torch.float64).reshape(B, 8 * A + 16)
        views = _greeks_views(block, A)
        assert set(views) == set(fields[:-4])
        names = basket_greeks_fields(A)
        assert len(names) == 2 * n + 4 == len(set(names))
        first = {"delta_put": 0, "delta_call": A, "vega_put": 2 * A, "vega_call": 3 * A, "rho_put": 4 * A, "rho_call": 4 * A + 1,
                 "theta_put": 4 * A + 2, "theta_call": 4 * A + 3, "correlation_put": 4 * A + 4, "correlation_call": 4 * A + 5}
        for name, col in first.items():
            per_asset = name.startswith(("delta", "vega"))
            for suffix, base in (("", 0), ("_stderr", n)):
                view = views[name + suffix]
                assert view.shape == ((B, A) if per_asset else (B,)), name
                assert view.data_ptr() == block[:, base + col].data_ptr(), name  # a view of the block, at its column
                assert torch.equal(view, block[:, base + col:base + col + A] if per_asset else block[:, base + col])
                assert names[base + col] == (f"{name}_0{suffix}" if per_asset else name + suffix)
        for j, name in enumerate(("put", "call", "put_stderr", "call_stderr")):
            assert views[name].data_ptr() == block[:, 2 * n + j].data_ptr() and names[2 * n + j] == name
    assert hasattr(BasketEngine, "greeks")


def test_basket_greeks_rejects_malformed_tensors_before_device_work() -> None:
    cfg = BasketConfig(n_assets=4, timesteps=16, network_size=64, batches_per_mc_run=32)
    good = torch.zeros((3, cfg.dim), dtype=torch.float64)
    for bad in (good.to(torch.float32), good[:, :cfg.dim - 1], torch.zeros((3, cfg.dim + 1), dtype=torch.float64),
                good.reshape(-1), good.reshape(3, 1, cfg.dim), torch.zeros((3, 2 * cfg.dim), dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match="contracts must be a contiguous"):
            basket_greeks(bad, cfg)
    for n in (0, -5):
        with pytest.raises(ValueError, match="n_paths"):
            basket_greeks(good, cfg, n_paths=n)
