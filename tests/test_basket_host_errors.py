"""The error surface of the basket entry points, replayed from tests/golden/basket_host_errors.json (recorded by
tests/golden/make_basket_host_errors.py from a library in which every entry point still carried its own copy of the
checks, so it holds the shared host layer of csrc/basket.hip to each entry's own behaviour): every status code and every last_error text of the recorded calls, which pin the order of the checks and the place of the
empty batch in each entry, and every recorded ``*_kernel`` name, which pins the mode rule and its parking bound per
kernel.  CPU only: no recorded call reaches a launch."""

from __future__ import annotations

import ctypes
import json
import os

from spectralmc_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basket_host_errors.json")
BATCHED = ("smc_basket_price", "smc_basket_price_general", "smc_basket_greeks", "smc_basket_greeks_general",
           "smc_basket_price_paths")


def _fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def _n_contracts(call: dict) -> int:
    return call["args"][5 if "general" in call["entry"] else 6 if "paths" in call["entry"] else 1]


def test_recorded_calls_answer_as_recorded() -> None:
    L = _lib.lib()
    dummy = (ctypes.c_double * 128)()
    buf = ctypes.addressof(dummy)
    calls = _fixture()["calls"]
    assert {c["entry"] for c in calls} == set(BATCHED) | {"smc_basket_train_targets"}
    for c in calls:
        # the record itself: nothing in it may reach a launch
        assert _n_contracts(c) == 0 or c["status"] in (_lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE), c
        assert (c["status"] == _lib.SMC_OK) == (c["error"] is None), c
        status = int(getattr(L, c["entry"])(*[buf if a == "buf" else a for a in c["args"]]))
        assert status == c["status"], c
        if status != _lib.SMC_OK:
            assert _lib.last_error() == c["error"], c
    assert all(v == 0.0 for v in dummy)


def test_recorded_calls_cover_every_check() -> None:
    """Each entry's record holds every message of its checks, on the empty batch and on one contract."""
    calls = _fixture()["calls"]
    shared = ("contracts_dev is NULL", "n_assets must be in 1..8", "bad math", "bad normalization",
              "need 0 <= n_contracts < 2^31", "n_paths too large")
    for entry in BATCHED:
        want = shared + (("greeks_dev is NULL",) if "greeks" in entry else ("prices_dev is NULL",))
        want += () if entry in ("smc_basket_price", "smc_basket_greeks") else ("weights_stride", "corr_stride")
        want += ("scales do not fit",) if entry == "smc_basket_price_paths" else ()
        for B in (0, 1):
            texts = [c["error"] for c in calls if c["entry"] == entry and c["error"] and _n_contracts(c) == B]
            assert all(t.startswith(entry + ": ") for t in texts)
            for part in want:
                assert any(part in t for t in texts), (entry, B, part)
        assert any(c["entry"] == entry and c["status"] == _lib.SMC_OK for c in calls)
    train = {c["error"] for c in calls if c["entry"] == "smc_basket_train_targets" and c["error"]}
    assert all(t.startswith("smc_basket_train_targets: ") for t in train)
    for part in ("NULL buffer", "n_assets must be in 1..8", "need 0 <= B < 2^31", "need N % 4 == 0", "bad math",
                 "bad store_mode", "path_pitch must be", "chunk_contracts <= 0"):  # the checks before any device query
        assert any(part in t for t in train), part


def test_recorded_kernel_names() -> None:
    L = _lib.lib()
    fx = _fixture()
    names = fx["names"]
    for entry in BATCHED:
        for A in range(1, 9):
            rows = [r for r in names if r[0] == entry and r[1] == A]
            taken = [r for r in rows if r[-1] != "unsupported"]
            stem = {"smc_basket_price": "basket_price_kernel", "smc_basket_price_general": "basket_general_kernel",
                    "smc_basket_price_paths": "basket_path_kernel"}.get(entry, entry[4:] + "_kernel")
            modes = ("raw", "replay") if "paths" in entry else ("raw", "lds", "replay")
            assert {r[-1] for r in taken} == {f"{stem}({m})" for m in modes}, (entry, A)
            # P = 1, 2048 and the two sides of the parking bound; the path kernel's bound is in the dates
            assert len({r[3] for r in taken}) == (2 if "paths" in entry else 4)
            assert len({r[2] for r in rows}) >= (3 if "paths" in entry else 1)
    for *query, name in names:
        assert getattr(L, query[0] + "_kernel")(*query[1:]).decode() == name, query
    assert {r[-1] for r in fx["train_names"]} == {"basket_resident_kernel", "basket_kernel+basket_cf_kernel",
                                                 "basket_kernel"}
    for *query, name in fx["train_names"]:
        assert L.smc_basket_train_targets_kernel(*query).decode() == name, query
