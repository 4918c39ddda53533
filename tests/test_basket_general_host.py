"""smc_basket_price_general / smc_basket_price_general_kernel on the host: argument errors come back as status codes
(with a last_error text that names the argument) before any HIP call and before the empty batch is accepted, the two
stride checks among them; the kernel name follows the flags and the parking bound; the binding's constants match
the header (ABI 21); basket_price rejects malformed weights and correlations before any device work; validate=True's
checks, run on CPU tensors; pack_correlation's index order.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from spectralmc_amd import _lib
from spectralmc_amd.basket import (BasketConfig, BasketEngine, basket_price, pack_correlation,
                                   validate_basket_inputs)
from tests.helpers import basket_general_cases as cases

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
PARK = 144 * 1024
SCRATCH = 2112  # bytes of this kernel's scratch at the head of the dynamic LDS (the header states it)


def _call(L, contracts, B, A, T, P, math, norm, out, tsum=None, w=None, ws=0, c=None, cs=0) -> int:
    return int(L.smc_basket_price_general(contracts, w, ws, c, cs, B, A, T, P, 7, None, 0, math, norm, out, tsum, None))


def test_general_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 18)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    for B in (1, 0):  # the errors are checked before the empty batch is accepted
        for tsum in (None, p):
            for w, c in ((None, None), (p, p)):
                kw = dict(w=w, ws=4, c=c, cs=6)
                assert _call(L, None, B, 4, 16, 1024, 0, NORM, p, tsum, **kw) == arg
                assert "smc_basket_price_general" in _lib.last_error() and "contracts_dev" in _lib.last_error()
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
            # the strides: 0 or at least a row, and only where the table is given
            for ws in (1, 3, -1, -4):
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, tsum, w=p, ws=ws) == arg, ws
                assert "weights_stride" in _lib.last_error()
            for cs in (1, 5, -1, -6):
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, tsum, c=p, cs=cs) == arg, cs
                assert "corr_stride" in _lib.last_error()
            # both wrong: the weights are named first; smc_basket_price's checks come before either
            assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, tsum, w=p, ws=3, c=p, cs=5) == arg
            assert "weights_stride" in _lib.last_error()
            assert _call(L, p, B, 4, 0, 1024, 0, NORM, p, tsum, w=p, ws=3, c=p, cs=5) == shape
            assert "timesteps" in _lib.last_error()
            assert _call(L, p, B, 9, 16, 1024, 0, NORM, p, tsum, w=p, ws=3, c=p, cs=5) == arg
            assert "n_assets" in _lib.last_error()
        for bad_b in (-1, 1 << 31, 1 << 40):
            assert _call(L, p, bad_b, 4, 16, 1024, 0, NORM, p) == shape, bad_b
            assert "n_contracts" in _lib.last_error()
    assert all(v == 0.0 for v in dummy)


def test_general_zero_contracts_is_a_noop() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 18)()
    p = ctypes.addressof(dummy)
    for A in range(1, 9):
        n = A * (A - 1) // 2
        for norm in (RAW, NORM):
            for math in (0, _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.MATH_HW | _lib.PRICE_REPLAY):
                for tsum in (None, p):
                    for T, P in ((16, 1024), (1, 1), (5, 693), (16, (1 << 40) - 1)):
                        assert _call(L, p, 0, A, T, P, math, norm, p, tsum) == _lib.SMC_OK
                        # every stride the call takes: shared rows, packed rows, padded rows; an ignored stride
                        for ws, cs in ((0, 0), (A, n), (A + 3, n + 5)):
                            assert _call(L, p, 0, A, T, P, math, norm, p, tsum, w=p, ws=ws, c=p, cs=cs) == _lib.SMC_OK
                        assert _call(L, p, 0, A, T, P, math, norm, p, tsum, w=None, ws=-7, c=None, cs=-7) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_general_kernel_names() -> None:
    L = _lib.lib()

    def name(A, T, P, math, norm) -> str:
        return L.smc_basket_price_general_kernel(A, T, P, math, norm).decode()

    lds, replay_name, raw = (f"basket_general_kernel({m})" for m in ("lds", "replay", "raw"))
    hw, replay = _lib.MATH_HW, _lib.PRICE_REPLAY
    for A in range(1, 9):
        for math in (0, hw, replay, hw | replay):
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20), (16, (1 << 40) - 1)):
                assert name(A, T, P, math, RAW) == raw
        for math in (replay, hw | replay):
            for T, P in ((16, 4096), (1, 1), (40, 693), (5, 1 << 20)):
                assert name(A, T, P, math, NORM) == replay_name
        for math in (0, hw):
            assert name(A, 3, 1, math, NORM) == lds
            assert name(A, 3, 693, math, NORM) == lds
    for math in (0, hw):
        assert name(4, 16, 8192, math, NORM) == lds            # 128 KiB parked
        assert name(4, 16, 131072, math, NORM) == replay_name  # 2 MiB
    # one switch from lds to replay per asset count, exactly where block + scratch pass the parking bound
    for A in range(1, 9):
        lo = 128 * 1024 // (4 * A) - 64
        ps = list(range(lo - lo % 4 + 1, PARK // (4 * A) + 64))
        names = [name(A, 16, P, 0, NORM) for P in ps]
        assert names[0] == lds and names[-1] == replay_name
        edge = names.index(replay_name)
        assert names[:edge] == [lds] * edge and names[edge:] == [replay_name] * (len(names) - edge)
        parked = [A * ((P + 3) // 4 * 4) * 4 + SCRATCH for P in ps]
        assert max(parked[:edge]) <= PARK < parked[edge], A
        assert [n == lds for n in names] == [b <= PARK for b in parked], A
        assert {name(A, 16, P, 0, NORM) for P in (1, 2, 3, 4, 5, 2047, 2048, 2049, ps[0] - 1)} == {lds}
        assert {name(A, 16, P, 0, NORM) for P in (ps[-1] + 1, 1 << 20, (1 << 40) - 1)} == {replay_name}
        # the same scratch as the price kernel's: the same switch
        price = [L.smc_basket_price_kernel(A, 16, P, 0, NORM).decode() for P in ps]
        assert [n.replace("price", "general") for n in price] == names
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


def test_general_constants_match_the_header() -> None:
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == 21 == int(re.search(r"#define\s+SMC_ABI_VERSION\s+(\w+)", text).group(1))
    assert _lib.lib().smc_abi_version() == 21
    assert _lib.BASKET_PRICE_COLS == 18
    sig = _lib.SIGNATURES["smc_basket_price_general"]
    assert sig[0] is ctypes.c_int32 and len(sig[1]) == 17
    # smc_basket_price's arguments with (weights, stride, corr, stride) after the contracts
    assert sig[1][:1] + sig[1][5:] == _lib.SIGNATURES["smc_basket_price"][1]
    assert sig[1][1:5] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    assert _lib.SIGNATURES["smc_basket_price_general_kernel"] == _lib.SIGNATURES["smc_basket_price_kernel"]
    decl = re.search(r"int32_t smc_basket_price_general\((.*?)\);", text, flags=re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 17
    assert f"{SCRATCH} bytes" in text[text.index("(ABI 21)"):]
    # the Python surface: the keywords of basket_price and of BasketEngine.price
    params = inspect.signature(basket_price).parameters
    assert list(params)[-3:] == ["weights", "correlation", "validate"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("weights", "correlation", "validate"))
    assert params["weights"].default is None and params["correlation"].default is None
    assert params["validate"].default is False
    eng = inspect.signature(BasketEngine.price).parameters
    assert eng["weights"].default is None and eng["correlation"].default is None


def test_basket_price_rejects_malformed_weights_and_correlation_before_device_work() -> None:
    A, B = 4, 3
    cfg = BasketConfig(n_assets=A, timesteps=16, network_size=64, batches_per_mc_run=32)
    good = torch.zeros((B, cfg.dim), dtype=torch.float64)
    w = torch.full((B, A), 0.25, dtype=torch.float64)
    for bad in (w.to(torch.float32), w[:, :3], torch.zeros((B + 1, A), dtype=torch.float64), w.reshape(-1),
                w.reshape(B, 1, A), torch.zeros((B, 2 * A), dtype=torch.float64)[:, ::2],
                torch.zeros(A + 1, dtype=torch.float64), w.numpy(), [0.25] * A):
        with pytest.raises(ValueError, match="weights must be a contiguous float64"):
            basket_price(good, cfg, weights=bad)
    C = torch.eye(A, dtype=torch.float64)
    tri = torch.zeros(6, dtype=torch.float64)
    for bad in (C.to(torch.float32), C[:3], C[:, :3], torch.zeros((B + 1, A, A), dtype=torch.float64),
                torch.zeros((B, A, A + 1), dtype=torch.float64), torch.zeros(5, dtype=torch.float64),
                torch.zeros((B, 7), dtype=torch.float64), torch.zeros((A, 2 * A), dtype=torch.float64)[:, ::2],
                torch.zeros((B, 12), dtype=torch.float64)[:, ::2], C.numpy()):
        with pytest.raises(ValueError, match="correlation must be a contiguous float64"):
            basket_price(good, cfg, correlation=bad)
    # well-formed tensors in host memory: named before the device is asked for
    with pytest.raises(ValueError, match="weights must be a device tensor"):
        basket_price(good, cfg, weights=w)
    with pytest.raises(ValueError, match="weights must be a device tensor"):
        basket_price(good, cfg, weights=w[0].contiguous(), correlation=C)
    for host in (C, C.expand(B, A, A).contiguous(), tri, tri.expand(B, 6).contiguous()):
        with pytest.raises(ValueError, match="correlation must be a device tensor"):
            basket_price(good, cfg, correlation=host)
    # the contracts are still looked at first
    with pytest.raises(ValueError, match="contracts must be a contiguous"):
        basket_price(good.to(torch.float32), cfg, weights=w.to(torch.float32))


def test_validate_rejections_on_cpu_tensors() -> None:
    """validate=True is validate_basket_inputs on the same tensors: run here on CPU-resident ones."""
    A = 4
    rng = np.random.default_rng(5)
    C = torch.from_numpy(cases.correlations(rng, 3, A))
    w = torch.from_numpy(rng.dirichlet(np.ones(A), 3))
    for ww, cc in ((w, C), (w[0], C[0]), (None, C), (w, None), (-w, pack_correlation(C)), (w, pack_correlation(C[0])),
                   (None, None)):
        validate_basket_inputs(ww, cc, A)
    for bad in (float("nan"), float("inf"), -float("inf")):
        w2 = w.clone()
        w2[1, 2] = bad
        with pytest.raises(ValueError, match="weights must be finite"):
            validate_basket_inputs(w2, C, A)
    asym = C.clone()
    asym[1, 2, 0] += 1e-9
    with pytest.raises(ValueError, match="symmetric"):
        validate_basket_inputs(w, asym, A)
    diag = C.clone()
    diag[2, 1, 1] = 1.0 + 1e-9
    with pytest.raises(ValueError, match="unit diagonal"):
        validate_basket_inputs(w, diag, A)
    indef = C.clone()
    indef[0] = torch.full((A, A), -0.5, dtype=torch.float64)  # equicorrelation below -1 / (A - 1)
    indef[0].fill_diagonal_(1.0)
    with pytest.raises(ValueError, match="positive definite"):
        validate_basket_inputs(w, indef, A)
    with pytest.raises(ValueError, match="positive definite"):
        validate_basket_inputs(w, pack_correlation(indef), A)
    with pytest.raises(ValueError, match="positive definite"):
        validate_basket_inputs(None, torch.ones((A, A), dtype=torch.float64), A)  # singular
    nan = C.clone()
    nan[0, 1, 0] = nan[0, 0, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        validate_basket_inputs(w, nan, A)
    # A = 3, where a [3, 3] tensor could be read as three packed rows: it is a matrix
    three = torch.tensor([[1.0, 0.1, 0.2], [0.3, 1.0, 0.1], [0.2, 0.1, 1.0]], dtype=torch.float64)
    with pytest.raises(ValueError, match="symmetric"):
        validate_basket_inputs(None, three, 3)


def test_pack_correlation_index_order() -> None:
    C = torch.arange(16, dtype=torch.float64).reshape(4, 4)  # entry (i, k) is 4 i + k: all distinct
    want = [4.0, 8.0, 9.0, 12.0, 13.0, 14.0]                 # (1,0), (2,0), (2,1), (3,0), (3,1), (3,2)
    got = pack_correlation(C)
    assert got.shape == (6,) and got.dtype == torch.float64 and got.is_contiguous() and got.tolist() == want
    for i in range(4):
        for k in range(i):
            assert got[i * (i - 1) // 2 + k] == C[i, k]     # the header's index
    batch = torch.stack([C, C + 100.0, -C])
    gb = pack_correlation(batch)
    assert gb.shape == (3, 6) and gb.is_contiguous()
    assert gb.tolist() == [want, [v + 100.0 for v in want], [-v for v in want]]
    np.testing.assert_array_equal(gb.numpy(), cases.pack(batch.numpy()))
    assert pack_correlation(torch.ones((1, 1), dtype=torch.float64)).shape == (0,)
    assert pack_correlation(torch.ones((5, 1, 1), dtype=torch.float64)).shape == (5, 0)
    for A in range(2, 9):
        M = torch.from_numpy(np.random.default_rng(A).standard_normal((2, A, A)))
        np.testing.assert_array_equal(pack_correlation(M).numpy(), cases.pack(M.numpy()))
    for bad in (torch.zeros(6), torch.zeros((2, 3)), torch.zeros((2, 2, 3, 3))):
        with pytest.raises(ValueError, match="correlation matrix"):
            pack_correlation(bad)
