"""smc_basket_greeks_paths / smc_basket_greeks_paths_kernel / smc_basket_greeks_paths_cols on the host: argument errors
come back as status codes (with a last_error text that names the argument) in smc_basket_price_paths' order, then the
table check in both normalisations, all before any HIP call and before the empty batch is accepted; the kernel name
follows the normalisation and is "unsupported" for every rejected call; the binding's surface matches the header;
basket_greeks_paths rejects malformed inputs before any device work, and validate=True is the only path that reads
values.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import inspect
import os
import re

import pytest
import torch

from spectralmc_amd import _lib, basket
from spectralmc_amd.basket import (PATH_GREEK_PAYOFFS, BasketConfig, BasketEngine, BasketPathGreeks, basket_greeks_paths,
                                   basket_path_greeks_fields)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
LDS = 144 * 1024
SCRATCH = 3328  # bytes of scratch at the head of the dynamic LDS (the header states it)
ROW = 512 * 8   # one row of per-lane f64 accumulators


def _fits(A: int, T: int) -> bool:
    """The header's rule: the scratch, the (3A + 1) T f32 table entries (padded to 8 bytes) and one date (2A rows) of
    accumulators."""
    return SCRATCH + ((3 * A + 1) * T * 4 + 7) // 8 * 8 + 2 * A * ROW <= LDS


def _call(L, contracts, B, A, T, P, math, norm, out, w=None, ws=0, c=None, cs=0) -> int:
    return int(L.smc_basket_greeks_paths(contracts, w, ws, c, cs, B, A, T, P, 7, None, 0, math, norm, out, None))


def test_path_greeks_argument_errors_do_not_launch_and_keep_their_order() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 152)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    for B in (1, 0):  # the errors are checked before the empty batch is accepted
        for norm0 in (NORM, RAW):
            for w, c in ((None, None), (p, p)):
                kw = dict(w=w, ws=4, c=c, cs=6)
                assert _call(L, None, B, 4, 16, 1024, 0, norm0, p, **kw) == arg
                assert "smc_basket_greeks_paths" in _lib.last_error() and "contracts_dev" in _lib.last_error()
                assert _call(L, p, B, 4, 16, 1024, 0, norm0, None, **kw) == arg
                assert "greeks_dev" in _lib.last_error()
                assert _call(L, None, B, 4, 16, 1024, 0, norm0, None, **kw) == arg
                assert "contracts_dev" in _lib.last_error()
                for A in (0, 9, -1, 64):
                    assert _call(L, p, B, A, 16, 1024, 0, norm0, p, **kw) == arg, A
                    assert "n_assets" in _lib.last_error()
                for norm in (7, -1, 2):
                    assert _call(L, p, B, 4, 16, 1024, 0, norm, p, **kw) == arg, norm
                    assert "normalization" in _lib.last_error()
                for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | _lib.MATH_HW, 1, 0x2000, -1,
                             _lib.MATH_HW | _lib.PRICE_REPLAY | _lib.TRAIN_DYNAMIC):
                    assert _call(L, p, B, 4, 16, 1024, math, norm0, p, **kw) == arg, math
                    assert "math" in _lib.last_error()
                assert _call(L, p, B, 9, 16, 1024, 1, 7, p, **kw) == arg and "n_assets" in _lib.last_error()
                assert _call(L, p, B, 4, 16, 1024, 1, 7, p, **kw) == arg and "math" in _lib.last_error()
                for T in (0, -3):
                    assert _call(L, p, B, 4, T, 1024, 0, norm0, p, **kw) == shape, T
                    assert "timesteps" in _lib.last_error()
                for P in (0, -8, 1 << 40, 1 << 62):
                    assert _call(L, p, B, 4, 16, P, 0, norm0, p, **kw) == shape, P
                    assert "n_paths" in _lib.last_error()
            for ws in (1, 3, -1, -4):
                assert _call(L, p, B, 4, 16, 1024, 0, norm0, p, w=p, ws=ws) == arg, ws
                assert "weights_stride" in _lib.last_error()
            for cs in (1, 5, -1, -6):
                assert _call(L, p, B, 4, 16, 1024, 0, norm0, p, c=p, cs=cs) == arg, cs
                assert "corr_stride" in _lib.last_error()
            # the order: the price call's checks, the weights' stride, the correlation's, then the tables
            big = 40000
            assert not _fits(4, big)
            assert _call(L, p, B, 4, big, 1024, 0, norm0, p, w=p, ws=3, c=p, cs=5) == arg
            assert "weights_stride" in _lib.last_error()
            assert _call(L, p, B, 4, big, 1024, 0, norm0, p, c=p, cs=5) == arg
            assert "corr_stride" in _lib.last_error()
            assert _call(L, p, B, 4, big, 1024, 0, norm0, p, w=p, ws=4, c=p, cs=6) == shape
            assert "tables" in _lib.last_error() and "timesteps" in _lib.last_error()
            assert _call(L, p, B, 4, big, 0, 0, norm0, p) == shape
            assert "n_paths" in _lib.last_error()
            assert _call(L, p, B, 9, big, 1024, 0, norm0, p, w=p, ws=3) == arg
            assert "n_assets" in _lib.last_error()
        for bad_b in (-1, 1 << 31, 1 << 40):
            assert _call(L, p, bad_b, 4, 16, 1024, 0, NORM, p) == shape, bad_b
            assert "n_contracts" in _lib.last_error()
    assert all(v == 0.0 for v in dummy)


def test_path_greeks_table_bound_in_both_normalisations() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 152)()
    p = ctypes.addressof(dummy)
    for A in range(1, 9):
        edge = max(T for T in range(1, LDS // (4 * (3 * A + 1)) + 2) if _fits(A, T))
        assert edge > 300
        for T in (1, 16, 40, edge - 1, edge):
            for math in (0, _lib.MATH_HW):
                for norm, label in ((RAW, b"raw"), (NORM, b"replay")):
                    assert _call(L, p, 0, A, T, 693, math, norm, p) == _lib.SMC_OK, (A, T)
                    assert L.smc_basket_greeks_paths_kernel(A, T, 693, math, norm) == b"basket_path_greeks_kernel(" + \
                        label + b")"
        for T in (edge + 1, edge + 2, 2 * edge, (1 << 31) - 1):
            for norm in (RAW, NORM):
                for B in (0, 1):
                    assert _call(L, p, B, A, T, 693, 0, norm, p) == _lib.SMC_ERR_INVALID_SHAPE, (A, T)
                    assert "tables" in _lib.last_error()
                assert L.smc_basket_greeks_paths_kernel(A, T, 693, 0, norm) == b"unsupported"
    assert all(v == 0.0 for v in dummy)


def test_path_greeks_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 152)()
    p = ctypes.addressof(dummy)
    for A in range(1, 9):
        n = A * (A - 1) // 2
        for norm in (RAW, NORM):
            for math in (0, _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.MATH_HW | _lib.PRICE_REPLAY):
                for T, P in ((16, 1024), (1, 1), (5, 693), (16, (1 << 40) - 1)):
                    assert _call(L, p, 0, A, T, P, math, norm, p) == _lib.SMC_OK
                    for ws, cs in ((0, 0), (A, n), (A + 3, n + 5)):
                        assert _call(L, p, 0, A, T, P, math, norm, p, w=p, ws=ws, c=p, cs=cs) == _lib.SMC_OK
                    assert _call(L, p, 0, A, T, P, math, norm, p, ws=-7, cs=-7) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_path_greeks_kernel_names_and_cols() -> None:
    L = _lib.lib()

    def name(A, T, P, math, norm) -> str:
        return L.smc_basket_greeks_paths_kernel(A, T, P, math, norm).decode()

    hw, replay = _lib.MATH_HW, _lib.PRICE_REPLAY
    for A in range(1, 9):
        assert L.smc_basket_greeks_paths_cols(A) == 16 * A + 24 == _lib.basket_path_greeks_cols(A)
        for math in (0, hw, replay, hw | replay):  # SMC_PRICE_REPLAY is accepted and changes nothing
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20), (16, (1 << 40) - 1), (16, 131072)):
                assert name(A, T, P, math, RAW) == "basket_path_greeks_kernel(raw)"
                assert name(A, T, P, math, NORM) == "basket_path_greeks_kernel(replay)"
    for A in (0, 9, -1, 64):
        assert L.smc_basket_greeks_paths_cols(A) == -1
        with pytest.raises(ValueError, match="n_assets must be in 1..8"):
            _lib.basket_path_greeks_cols(A)
    assert _lib.basket_path_greeks_cols(1) == _lib.PATH_GREEKS_COLS  # smc_gbm_greeks_paths' 40-column layout
    for norm in (RAW, NORM):
        for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | hw, 1, 0x2000, -1):
            assert name(4, 16, 4096, math, norm) == "unsupported", math
        for A in (0, 9, -1):
            assert name(A, 16, 4096, 0, norm) == "unsupported", A
        for T, P in ((0, 4096), (-1, 4096), (16, 0), (16, -4), (16, 1 << 40)):
            assert name(4, T, P, 0, norm) == "unsupported"
        assert name(8, 4000, 2048, 0, norm) == "unsupported"
    assert name(4, 16, 4096, 0, 7) == "unsupported"
    assert name(4, 16, 4096, 0, -1) == "unsupported"


def test_path_greeks_surface_matches_the_header() -> None:
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+SMC_ABI_VERSION\s+(\w+)", text).group(1))
    sig = _lib.SIGNATURES["smc_basket_greeks_paths"]
    assert sig[0] is ctypes.c_int32 and len(sig[1]) == 16
    # smc_basket_price_paths' arguments without the barriers and the terminal sums
    price = _lib.SIGNATURES["smc_basket_price_paths"][1]
    assert sig[1] == price[:5] + price[6:16] + price[17:]
    assert _lib.SIGNATURES["smc_basket_greeks_paths_kernel"] == _lib.SIGNATURES["smc_basket_price_paths_kernel"]
    assert _lib.SIGNATURES["smc_basket_greeks_paths_cols"] == _lib.SIGNATURES["smc_basket_greeks_general_cols"]
    decl = re.search(r"int32_t smc_basket_greeks_paths\((.*?)\);", text, flags=re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 16
    section = text[text.index("Greeks of the Asian and lookback basket options"):]
    assert f"{SCRATCH} bytes of scratch" in section
    for phrase in ("Greeks of these payoffs", "basket path Greeks"):
        assert phrase not in text
    for phrase in ("correlation-pair sensitivities", "knock-out and worst-of Greeks", "gammas",
                   "sensitivities to the weights", "terminal_sum_dev", "float64 basket engine",
                   "continuous-monitoring corrections"):
        assert phrase in section.replace("\n * ", " "), phrase


def test_path_greeks_fields_and_views() -> None:
    assert PATH_GREEK_PAYOFFS == ("asian_put", "asian_call", "lookback_put", "lookback_call")
    for A in range(1, 9):
        names = basket_path_greeks_fields(A)
        G = 2 * A + 2
        assert len(names) == 16 * A + 24 == len(set(names))
        for g in range(G):
            kind = "delta" if g < A else "vega" if g < 2 * A else "rho" if g == 2 * A else "theta"
            tail = f"_{g % A}" if g < 2 * A else ""
            for q, pay in enumerate(PATH_GREEK_PAYOFFS):
                assert names[4 * g + q] == f"{kind}_{pay}{tail}"
                assert names[4 * G + 4 * g + q] == f"{kind}_{pay}{tail}_stderr"
        for q, pay in enumerate(PATH_GREEK_PAYOFFS):
            assert names[8 * G + q] == pay and names[8 * G + 4 + q] == pay + "_stderr"
        B = 3
        block = torch.arange(B * (16 * A + 24), dtype=torch.float64).reshape(B, 16 * A + 24)
        res = BasketPathGreeks(**basket._path_greeks_views(block, A), block=block)
        for q, pay in enumerate(PATH_GREEK_PAYOFFS):
            for suffix, base in (("", 0), ("_stderr", 4 * G)):
                d, v = getattr(res, f"delta_{pay}{suffix}"), getattr(res, f"vega_{pay}{suffix}")
                assert d.shape == v.shape == (B, A)
                for i in range(A):
                    assert torch.equal(d[:, i], block[:, base + 4 * i + q])
                    assert torch.equal(v[:, i], block[:, base + 4 * (A + i) + q])
                assert torch.equal(getattr(res, f"rho_{pay}{suffix}"), block[:, base + 8 * A + q])
                assert torch.equal(getattr(res, f"theta_{pay}{suffix}"), block[:, base + 8 * A + 4 + q])
            assert torch.equal(getattr(res, pay), block[:, 8 * G + q])
            assert torch.equal(getattr(res, pay + "_stderr"), block[:, 8 * G + 4 + q])
            assert getattr(res, f"delta_{pay}").data_ptr() == block.data_ptr() + 8 * q  # views, not copies
    with pytest.raises(ValueError, match="n_assets must be in 1..8"):
        basket_path_greeks_fields(9)
    assert BasketPathGreeks.__dataclass_params__.frozen
    fields = [f.name for f in BasketPathGreeks.__dataclass_fields__.values()]
    assert fields[-1] == "block" and len(fields) == 41
    params = inspect.signature(basket_greeks_paths).parameters
    assert list(params) == ["contracts", "cfg", "weights", "correlation", "ordinal0", "n_paths", "validate"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[2:])
    assert [params[k].default for k in list(params)[2:]] == [None, None, 0, None, False]
    eng = inspect.signature(BasketEngine.greeks_paths).parameters
    assert all(eng[k].default == params[k].default for k in list(params)[2:])
    for name in ("PATH_GREEK_PAYOFFS", "BasketPathGreeks", "basket_greeks_paths", "basket_path_greeks_fields"):
        assert name in basket.__all__


def test_basket_greeks_paths_rejects_malformed_inputs_before_device_work() -> None:
    A, B = 4, 3
    cfg = BasketConfig(n_assets=A, timesteps=16, network_size=64, batches_per_mc_run=32)
    good = torch.zeros((B, cfg.dim), dtype=torch.float64)
    w = torch.full((B, A), 0.25, dtype=torch.float64)
    for bad in (w.to(torch.float32), w[:, :3], torch.zeros((B + 1, A), dtype=torch.float64), w.reshape(-1), w.numpy()):
        with pytest.raises(ValueError, match="weights must be a contiguous float64"):
            basket_greeks_paths(good, cfg, weights=bad)
    C = torch.eye(A, dtype=torch.float64)
    for bad in (C.to(torch.float32), C[:3], torch.zeros((B + 1, A, A), dtype=torch.float64),
                torch.zeros(5, dtype=torch.float64), C.numpy()):
        with pytest.raises(ValueError, match="correlation must be a contiguous float64"):
            basket_greeks_paths(good, cfg, correlation=bad)
    with pytest.raises(ValueError, match="weights must be a device tensor"):
        basket_greeks_paths(good, cfg, weights=w, correlation=C)
    with pytest.raises(ValueError, match="correlation must be a device tensor"):
        basket_greeks_paths(good, cfg, correlation=C)
    with pytest.raises(ValueError, match="contracts must be a contiguous"):
        basket_greeks_paths(good.to(torch.float32), cfg)
    with pytest.raises(ValueError, match="n_paths must be positive"):
        basket_greeks_paths(good, cfg, n_paths=0)


def test_validate_is_the_only_path_that_reads_values(monkeypatch) -> None:
    """basket_greeks_paths hands `validate` to the shared checks, which look at the values (a synchronisation for
    device tensors) only when it is set: seen here with the device requirement and the library call stubbed out."""
    A, B = 2, 3
    cfg = BasketConfig(n_assets=A, timesteps=4, network_size=64, batches_per_mc_run=32)
    seen: list[str] = []

    monkeypatch.setattr(basket, "validate_basket_inputs", lambda w, c, a: seen.append("inputs"))
    monkeypatch.setattr(basket, "validate_basket_barriers", lambda b: seen.append("barriers"))
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    good = torch.zeros((B, cfg.dim), dtype=torch.float64)
    for validate in (False, True):
        seen.clear()
        with pytest.raises(ValueError, match="contracts must be a device tensor"):
            basket_greeks_paths(good, cfg, validate=validate)
        assert seen == []  # placement is checked before the values are looked at
    src = inspect.getsource(basket_greeks_paths)
    assert "synchronize" not in src and ".cpu()" not in src and ".item()" not in src
    assert "_batched_call(contracts, cfg, n_paths, weights, correlation, validate)" in src
    shared = inspect.getsource(basket._batched_call)
    assert shared.count("validate_basket_inputs(") == 1 and "if validate:" in shared
