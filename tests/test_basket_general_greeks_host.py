"""smc_basket_greeks_general and its two queries on the host: the symbols and their signatures; the column count; the
kernel name over flags and the parking bound (this kernel's scratch, which the header states); argument errors as
status codes before any HIP call and before the empty batch; basket_greeks' checks of weights and correlation before
device work; unpack_correlation; the field names and view shapes of BasketGeneralGreeks; calls without the new
arguments still bind smc_basket_greeks.  CPU only (no kernel launches)."""

from __future__ import annotations

import ctypes
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

import spectralmc_amd.basket as basket_mod
from spectralmc_amd import _lib
from spectralmc_amd.basket import (BasketConfig, BasketEngine, BasketGeneralGreeks, BasketGreeks,
                                   basket_general_greeks_fields, basket_greeks, basket_greeks_fields, pack_correlation,
                                   unpack_correlation)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spectralmc_hip.h")
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
PARK = 144 * 1024
SCRATCH = 15968  # bytes of this kernel's scratch at the head of the dynamic LDS (the header states it)


def _call(L, contracts, B, A, T, P, math, norm, out, sums=None, w=None, ws=0, c=None, cs=0) -> int:
    return int(L.smc_basket_greeks_general(contracts, w, ws, c, cs, B, A, T, P, 7, None, 0, math, norm, out, sums, None))


def test_symbols_and_signatures() -> None:
    L = _lib.lib()
    text = open(HEADER).read()
    for name in ("smc_basket_greeks_general", "smc_basket_greeks_general_kernel", "smc_basket_greeks_general_cols"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    # additive under ABI 21, and said so next to the define
    assert _lib.ABI_VERSION == 21 == L.smc_abi_version()
    define = text.index("#define SMC_ABI_VERSION")
    assert "smc_basket_greeks_general" in text[define:define + 700] and "additive" in text[define:define + 700]
    sig = _lib.SIGNATURES["smc_basket_greeks_general"]
    # smc_basket_price_general's argument types (the outputs are two pointers there as here), and smc_basket_greeks's
    # with (weights, stride, corr, stride) after the contracts
    assert sig == _lib.SIGNATURES["smc_basket_price_general"] and len(sig[1]) == 17
    assert sig[1][:1] + sig[1][5:] == _lib.SIGNATURES["smc_basket_greeks"][1]
    assert sig[1][1:5] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    assert _lib.SIGNATURES["smc_basket_greeks_general_kernel"] == _lib.SIGNATURES["smc_basket_greeks_kernel"]
    assert _lib.SIGNATURES["smc_basket_greeks_general_cols"] == _lib.SIGNATURES["smc_basket_greeks_cols"]
    decl = re.search(r"int32_t smc_basket_greeks_general\((.*?)\);", text, flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert names == ["contracts_dev", "weights_dev", "weights_stride", "corr_dev", "corr_stride", "n_contracts",
                     "n_assets", "timesteps", "n_paths", "mc_seed", "ordinal_dev", "ordinal0", "math", "normalization",
                     "greeks_dev", "sums_dev", "stream"]
    # the new section stands after the ABI 21 section and states its scratch
    assert text.index("(ABI 21)") < text.index("smc_basket_price_general(") < text.index("smc_basket_greeks_general(")
    assert f"{SCRATCH} bytes" in text[text.index("additive under ABI 21"):]


def test_cols() -> None:
    L = _lib.lib()
    for A in range(0, 10):
        want = 2 * A * A + 6 * A + 12 if 1 <= A <= 8 else -1
        assert L.smc_basket_greeks_general_cols(A) == want
        if want > 0:
            pairs = A * (A - 1) // 2
            assert want == 2 * (4 * A + 4 + 2 * pairs) + 4 == _lib.basket_greeks_general_cols(A)
            assert len(basket_general_greeks_fields(A)) == want
        else:
            with pytest.raises(ValueError, match="n_assets"):
                _lib.basket_greeks_general_cols(A)
            with pytest.raises(ValueError, match="n_assets"):
                basket_general_greeks_fields(A)
    assert L.smc_basket_greeks_general_cols(-1) == -1


def test_kernel_names_and_the_parking_switch() -> None:
    L = _lib.lib()

    def name(A, T, P, math, norm) -> str:
        return L.smc_basket_greeks_general_kernel(A, T, P, math, norm).decode()

    lds, replay_name, raw = (f"basket_greeks_general_kernel({m})" for m in ("lds", "replay", "raw"))
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
    # one switch from lds to replay per asset count, exactly where block + scratch pass the parking bound
    for A in range(1, 9):
        lo = 112 * 1024 // (4 * A) - 64
        ps = list(range(lo - lo % 4 + 1, PARK // (4 * A) + 64))
        names = [name(A, 16, P, 0, NORM) for P in ps]
        assert names[0] == lds and names[-1] == replay_name
        edge = names.index(replay_name)
        assert names[:edge] == [lds] * edge and names[edge:] == [replay_name] * (len(names) - edge)
        parked = [A * ((P + 3) // 4 * 4) * 4 + SCRATCH for P in ps]
        assert max(parked[:edge]) <= PARK < parked[edge], A
        assert [n == lds for n in names] == [b <= PARK for b in parked], A
        assert [name(A, 16, P, hw, NORM) for P in ps] == names
        assert {name(A, 16, P, 0, NORM) for P in (1, 2, 3, 4, 5, 2047, 2048, 2049, ps[0] - 1)} == {lds}
        assert {name(A, 16, P, 0, NORM) for P in (ps[-1] + 1, 1 << 20, (1 << 40) - 1)} == {replay_name}
    for norm in (RAW, NORM):
        for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | hw, 1, 0x2000, -1):
            assert name(4, 16, 4096, math, norm) == "unsupported", math
        for A in (0, 9, -1):
            assert name(A, 16, 4096, 0, norm) == "unsupported", A
        for T, P in ((0, 4096), (-1, 4096), (16, 0), (16, -4), (16, 1 << 40)):
            assert name(4, T, P, 0, norm) == "unsupported"
    assert name(4, 16, 4096, 0, 7) == "unsupported"
    assert name(4, 16, 4096, 0, -1) == "unsupported"


def test_argument_errors_do_not_launch() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 68)()
    p = ctypes.addressof(dummy)
    arg, shape = _lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE
    for B in (1, 0):  # the errors are checked before the empty batch is accepted
        for sums in (None, p):
            for w, c in ((None, None), (p, p)):
                kw = dict(w=w, ws=4, c=c, cs=6)
                assert _call(L, None, B, 4, 16, 1024, 0, NORM, p, sums, **kw) == arg
                assert "smc_basket_greeks_general" in _lib.last_error() and "contracts_dev" in _lib.last_error()
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, None, sums, **kw) == arg
                assert "greeks_dev" in _lib.last_error()
                for A in (0, 9, -1, 64):
                    assert _call(L, p, B, A, 16, 1024, 0, NORM, p, sums, **kw) == arg, A
                    assert "n_assets" in _lib.last_error()
                for norm in (7, -1, 2):
                    assert _call(L, p, B, 4, 16, 1024, 0, norm, p, sums, **kw) == arg, norm
                    assert "normalization" in _lib.last_error()
                for math in (_lib.MATH_REF, _lib.TRAIN_DYNAMIC, _lib.MATH_REF | _lib.MATH_HW, 1, 0x2000, -1,
                             _lib.MATH_HW | _lib.PRICE_REPLAY | _lib.TRAIN_DYNAMIC):
                    assert _call(L, p, B, 4, 16, 1024, math, NORM, p, sums, **kw) == arg, math
                    assert "math" in _lib.last_error()
                for T in (0, -3):
                    assert _call(L, p, B, 4, T, 1024, 0, NORM, p, sums, **kw) == shape, T
                    assert "timesteps" in _lib.last_error()
                for P in (0, -8, 1 << 40, 1 << 62):
                    assert _call(L, p, B, 4, 16, P, 0, NORM, p, sums, **kw) == shape, P
                    assert "n_paths" in _lib.last_error()
            # the strides: 0 or at least a row, and only where the table is given
            for ws in (1, 3, -1, -4):
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, sums, w=p, ws=ws) == arg, ws
                assert "weights_stride" in _lib.last_error()
            for cs in (1, 5, -1, -6):
                assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, sums, c=p, cs=cs) == arg, cs
                assert "corr_stride" in _lib.last_error()
            # in order: the weights are named before the correlation, smc_basket_greeks's checks before either, and
            # within those the pointers, the asset count, the flags, then the shape
            assert _call(L, p, B, 4, 16, 1024, 0, NORM, p, sums, w=p, ws=3, c=p, cs=5) == arg
            assert "weights_stride" in _lib.last_error()
            assert _call(L, p, B, 4, 0, 1024, 0, NORM, p, sums, w=p, ws=3, c=p, cs=5) == shape
            assert "timesteps" in _lib.last_error()
            assert _call(L, p, B, 9, 16, 1024, 0, NORM, p, sums, w=p, ws=3, c=p, cs=5) == arg
            assert "n_assets" in _lib.last_error()
            assert _call(L, None, B, 9, 0, 0, 1, 7, None, sums, w=p, ws=3, c=p, cs=5) == arg
            assert "contracts_dev" in _lib.last_error()
            assert _call(L, p, B, 9, 0, 0, 1, 7, None, sums) == arg
            assert "greeks_dev" in _lib.last_error()
            assert _call(L, p, B, 4, 0, 0, 1, 7, p, sums) == arg
            assert "math" in _lib.last_error()
            assert _call(L, p, B, 4, 0, 0, 0, 7, p, sums) == arg
            assert "normalization" in _lib.last_error()
        for bad_b in (-1, 1 << 31, 1 << 40):
            assert _call(L, p, bad_b, 4, 16, 1024, 0, NORM, p) == shape, bad_b
            assert "n_contracts" in _lib.last_error()
    # the empty batch: SMC_OK, nothing touched, whatever strides the call takes
    for A in range(1, 9):
        n = A * (A - 1) // 2
        for norm in (RAW, NORM):
            for math in (0, _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.MATH_HW | _lib.PRICE_REPLAY):
                for ws, cs in ((0, 0), (A, n), (A + 3, n + 5)):
                    assert _call(L, p, 0, A, 5, 693, math, norm, p, p, w=p, ws=ws, c=p, cs=cs) == _lib.SMC_OK
                assert _call(L, p, 0, A, 5, 693, math, norm, p, None, w=None, ws=-7, c=None, cs=-7) == _lib.SMC_OK
    assert all(v == 0.0 for v in dummy)


def test_basket_greeks_rejects_malformed_weights_and_correlation_before_device_work() -> None:
    A, B = 4, 3
    cfg = BasketConfig(n_assets=A, timesteps=16, network_size=64, batches_per_mc_run=32)
    good = torch.zeros((B, cfg.dim), dtype=torch.float64)
    w = torch.full((B, A), 0.25, dtype=torch.float64)
    for bad in (w.to(torch.float32), w[:, :3], torch.zeros((B + 1, A), dtype=torch.float64), w.reshape(-1),
                w.reshape(B, 1, A), torch.zeros((B, 2 * A), dtype=torch.float64)[:, ::2],
                torch.zeros(A + 1, dtype=torch.float64), w.numpy(), [0.25] * A):
        with pytest.raises(ValueError, match="weights must be a contiguous float64"):
            basket_greeks(good, cfg, weights=bad)
    C = torch.eye(A, dtype=torch.float64)
    tri = torch.zeros(6, dtype=torch.float64)
    for bad in (C.to(torch.float32), C[:3], C[:, :3], torch.zeros((B + 1, A, A), dtype=torch.float64),
                torch.zeros((B, A, A + 1), dtype=torch.float64), torch.zeros(5, dtype=torch.float64),
                torch.zeros((B, 7), dtype=torch.float64), torch.zeros((A, 2 * A), dtype=torch.float64)[:, ::2],
                torch.zeros((B, 12), dtype=torch.float64)[:, ::2], C.numpy()):
        with pytest.raises(ValueError, match="correlation must be a contiguous float64"):
            basket_greeks(good, cfg, correlation=bad)
    # well-formed tensors in host memory: named before the device is asked for
    with pytest.raises(ValueError, match="weights must be a device tensor"):
        basket_greeks(good, cfg, weights=w)
    with pytest.raises(ValueError, match="weights must be a device tensor"):
        basket_greeks(good, cfg, weights=w[0].contiguous(), correlation=C)
    for host in (C, C.expand(B, A, A).contiguous(), tri, tri.expand(B, 6).contiguous()):
        with pytest.raises(ValueError, match="correlation must be a device tensor"):
            basket_greeks(good, cfg, correlation=host)
    # the contracts and the path count are still looked at first
    with pytest.raises(ValueError, match="contracts must be a contiguous"):
        basket_greeks(good.to(torch.float32), cfg, weights=w.to(torch.float32))
    with pytest.raises(ValueError, match="n_paths must be positive"):
        basket_greeks(good, cfg, n_paths=0, weights=w.to(torch.float32))
    # the keywords of basket_greeks and of BasketEngine.greeks
    params = inspect.signature(basket_greeks).parameters
    assert list(params)[-3:] == ["weights", "correlation", "validate"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("weights", "correlation", "validate"))
    assert params["weights"].default is None and params["correlation"].default is None
    assert params["validate"].default is False
    eng = inspect.signature(BasketEngine.greeks).parameters
    assert all(eng[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("weights", "correlation", "validate"))
    assert eng["weights"].default is None and eng["correlation"].default is None and eng["validate"].default is False


def test_unpack_correlation_round_trip() -> None:
    tri = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], dtype=torch.float64)  # (1,0), (2,0), (2,1), (3,0), (3,1), (3,2)
    M = unpack_correlation(tri, 4)
    assert M.shape == (4, 4) and M.dtype == torch.float64
    assert M.tolist() == [[0, 1, 2, 4], [1, 0, 3, 5], [2, 3, 0, 6], [4, 5, 6, 0]]
    for A in range(1, 9):
        n = A * (A - 1) // 2
        rows = torch.from_numpy(np.random.default_rng(A).standard_normal((3, 2, n)))
        full = unpack_correlation(rows, A)
        assert full.shape == (3, 2, A, A)
        assert torch.equal(full, full.transpose(-1, -2))
        assert bool((torch.diagonal(full, dim1=-2, dim2=-1) == 0.0).all())
        assert torch.equal(pack_correlation(full.reshape(6, A, A)), rows.reshape(6, n))
        for j in range(A):
            for k in range(j):
                assert torch.equal(full[..., j, k], rows[..., j * (j - 1) // 2 + k])
        # and the other way: a symmetric matrix less its diagonal
        C = torch.from_numpy(np.random.default_rng(10 + A).standard_normal((A, A)))
        C = C + C.T
        assert torch.equal(unpack_correlation(pack_correlation(C), A), C - torch.diag(torch.diagonal(C)))
    assert unpack_correlation(torch.zeros((5, 0), dtype=torch.float64), 1).shape == (5, 1, 1)
    for bad, A in ((torch.zeros(5), 4), (torch.zeros((2, 6)), 3), (torch.zeros(()), 1)):
        with pytest.raises(ValueError, match="packed rows"):
            unpack_correlation(bad, A)
    with pytest.raises(ValueError, match="n_assets"):
        unpack_correlation(torch.zeros(36), 9)


def test_field_names_and_view_shapes() -> None:
    for A in range(1, 9):
        names = basket_general_greeks_fields(A)
        pairs = A * (A - 1) // 2
        n = 4 * A + 4 + 2 * pairs
        assert len(names) == len(set(names)) == 2 * n + 4
        old = basket_greeks_fields(A)
        assert names[:4 * A + 4] == old[:4 * A + 4] and names[-4:] == old[-4:] == ("put", "call", "put_stderr", "call_stderr")
        want = [f"correlation_put_{j}_{k}" for j in range(A) for k in range(j)]
        assert list(names[4 * A + 4:4 * A + 4 + pairs]) == want
        assert list(names[4 * A + 4 + pairs:n]) == [w.replace("put", "call") for w in want]
        assert names[n:2 * n] == tuple(m + "_stderr" for m in names[:n])
        B = 3
        block = torch.arange(B * (2 * n + 4), dtype=torch.float64).reshape(B, 2 * n + 4)
        views = basket_mod._general_greeks_views(block, A)
        fields = [f.name for f in dataclasses.fields(BasketGeneralGreeks)]
        assert set(views) == set(fields) - {"terminal_sum", "sum_moments", "block"}
        # BasketGreeks's fields, with the moments in place of its two sums
        assert set(fields) - {"sum_moments"} == {f.name for f in dataclasses.fields(BasketGreeks)} - {"sum_xl", "sum_xc"}
        for name, view in views.items():
            per_asset = name.startswith(("delta", "vega"))
            per_pair = name.startswith("correlation")
            assert view.shape == ((B, A) if per_asset else (B, pairs) if per_pair else (B,)), name
            assert view.untyped_storage().data_ptr() == block.untyped_storage().data_ptr(), name
            # the view's columns are the block's columns of those names
            stem, tail = (name[:-7], "_stderr") if name.endswith("_stderr") else (name, "")
            if per_asset:
                want_cols = [names.index(f"{stem}_{i}{tail}") for i in range(A)]
            elif per_pair:
                want_cols = [names.index(f"{stem}_{j}_{k}{tail}") for j in range(A) for k in range(j)]
            else:
                want_cols = [names.index(name)]
            assert torch.equal(view.reshape(B, -1), block[:, want_cols]), name
    got = BasketGeneralGreeks(**basket_mod._general_greeks_views(torch.zeros((2, 68)), 4), terminal_sum=torch.zeros((2, 4)),
                              sum_moments=torch.zeros((2, 10)), block=torch.zeros((2, 68)))
    with pytest.raises(dataclasses.FrozenInstanceError):
        got.put = None  # type: ignore[misc]
    for name in ("BasketGeneralGreeks", "basket_general_greeks_fields", "unpack_correlation", "basket_greeks"):
        assert name in basket_mod.__all__


class _Recorder:
    """Stands in for the loaded library: records which entry point a call binds, launches nothing."""

    def __init__(self, real) -> None:
        self.calls: list[tuple[str, tuple]] = []
        self._real = real

    def __getattr__(self, name: str):
        real = getattr(self._real, name)
        if name in ("smc_basket_greeks", "smc_basket_greeks_general"):
            def record(*args):
                self.calls.append((name, args))
                return _lib.SMC_OK
            return record
        return real


def test_calls_without_the_new_arguments_still_bind_smc_basket_greeks(monkeypatch) -> None:
    A, B = 3, 2
    cfg = BasketConfig(n_assets=A, timesteps=4, network_size=64, batches_per_mc_run=32, normalize=True, math="portable")
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    monkeypatch.setattr(_lib, "stream_handle", lambda stream=None: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    rows = torch.zeros((B, cfg.dim), dtype=torch.float64)
    out = basket_greeks(rows, cfg, n_paths=100)
    assert isinstance(out, BasketGreeks) and out.block.shape == (B, 8 * A + 16)
    assert [c[0] for c in rec.calls] == ["smc_basket_greeks"] and len(rec.calls[0][1]) == 13
    w = torch.tensor([0.5, 0.25, 0.25], dtype=torch.float64)
    C = torch.eye(A, dtype=torch.float64).expand(B, A, A).contiguous()
    for kw, strides in (({"weights": w}, (0, 0)), ({"correlation": C}, (0, 3)), ({"weights": w, "correlation": C}, (0, 3)),
                        ({"weights": w.expand(B, A).contiguous(), "correlation": C[0].contiguous()}, (A, 0))):
        rec.calls.clear()
        got = basket_greeks(rows, cfg, n_paths=100, **kw)
        assert isinstance(got, BasketGeneralGreeks)
        assert [c[0] for c in rec.calls] == ["smc_basket_greeks_general"]
        args = rec.calls[0][1]
        assert len(args) == 17 and (args[2], args[4]) == strides and args[5:9] == (B, A, 4, 100)
        assert (args[1] is None) == ("weights" not in kw) and (args[3] is None) == ("correlation" not in kw)
        assert got.block.shape == (B, 2 * A * A + 6 * A + 12)
        assert got.correlation_put.shape == got.correlation_call_stderr.shape == (B, 3)
        assert got.terminal_sum.shape == (B, A) and got.sum_moments.shape == (B, 6)
        for view in (got.delta_put, got.put, got.correlation_call_stderr):
            assert view.untyped_storage().data_ptr() == got.block.untyped_storage().data_ptr()
