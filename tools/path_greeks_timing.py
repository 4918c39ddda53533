"""Timing of the batched Greeks of the Asian and lookback options (smc_gbm_greeks_paths, path_greeks_kernel) beside
the path-dependent pricer (smc_gbm_price_paths, path_price_kernel) at the same shape, math and normalisation in the
same process.  Needs a GPU.

    python tools/path_greeks_timing.py            # the record: profiles/path_greeks/timing.json

Windows of the record (T = 16, float32, B = 4096 contracts): P = 8192 and P = 65,536, hardware and portable math,
RAW and NORMALIZE: each pair warmed up, then the kernel's own execution time of --calls calls of each, alternating
call by call (smc_time_launches: each call alone on a drained stream; medians; ratio = Greeks / price).  Beside each
ratio stands the cost of the route the call replaces, bump and revalue: nine smc_gbm_price_paths calls (the base
and central differences in X0, v, r and T), i.e. 9 against the one pricing call.  The two calls' common columns
(the four prices and their standard errors) are checked to agree bit for bit before anything is timed."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spectralmc_amd import _lib  # noqa: E402
from tools.price_batch_timing import T, contracts, kernel_ms  # noqa: E402

BUMP_AND_REVALUE_CALLS = 9


def window(cd: torch.Tensor, P: int, math: str, norm: int, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    greeks = torch.empty((B, _lib.PATH_GREEKS_COLS), dtype=torch.float64, device=cd.device)
    prices = torch.empty((B, _lib.PATH_PRICE_COLS), dtype=torch.float64, device=cd.device)

    def call_greeks() -> None:
        _lib.check(L.smc_gbm_greeks_paths(_lib.ptr(cd), B, T, P, 7, None, 0, flag, norm, _lib.DTYPE_F32,
                                          _lib.ptr(greeks), _lib.stream_handle()))

    def call_price() -> None:
        _lib.check(L.smc_gbm_price_paths(_lib.ptr(cd), None, B, T, P, 7, None, 0, flag, norm, _lib.DTYPE_F32,
                                         _lib.ptr(prices), _lib.stream_handle()))

    for _ in range(warmup):
        call_greeks()
        call_price()
    torch.cuda.synchronize()
    assert torch.equal(greeks[:, 32:40], prices[:, [0, 1, 4, 5, 8, 9, 12, 13]]), "the two calls' common columns differ"
    kg, kp = [], []
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        kg += kernel_ms(call_greeks, 1)
        kp += kernel_ms(call_price, 1)

    def stats(name: str, k: list[float]) -> dict:
        return {"kernel": name, "kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
                "kernel_ms_max": round(max(k), 4)}

    ratio = statistics.median(kg) / statistics.median(kp)
    return {"window": "smc_gbm_greeks_paths beside smc_gbm_price_paths", "B": B, "T": T, "P": P, "dtype": "float32",
            "math": math, "normalization": "normalize" if norm == _lib.NORM_NORMALIZE else "raw", "calls_each": calls,
            "greeks": stats(L.smc_gbm_greeks_paths_kernel(T, P, flag, norm, _lib.DTYPE_F32).decode(), kg),
            "price": stats(L.smc_gbm_price_paths_kernel(T, P, flag, norm, _lib.DTYPE_F32).decode(), kp),
            "ratio_greeks_to_price": round(ratio, 3),
            "bump_and_revalue_price_calls": BUMP_AND_REVALUE_CALLS,
            "bump_and_revalue_over_greeks": round(BUMP_AND_REVALUE_CALLS / ratio, 3)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contracts", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per kernel and window (at least 10 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    _lib.require_device()
    cd = torch.tensor(contracts(args.contracts), dtype=torch.float64, device="cuda")
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/path_greeks_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION}
    windows = []
    for P in (8192, 65536):
        for math in ("hw", "portable"):
            for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
                windows.append(window(cd, P, math, norm, args.calls, args.warmup))
    record["windows"] = windows
    out = args.out or os.path.join(ROOT, "profiles", "path_greeks", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
