"""Timing of the batched pathwise Greeks (smc_gbm_greeks, greeks_kernel) beside the batched pricer
(smc_gbm_price, price_kernel) at the same shape, mode and math in the same process.  Needs a GPU.

    python tools/greeks_timing.py                 # the record: profiles/greeks/timing.json

Windows of the record (T = 16, float32, NORMALIZE, B = 4096 contracts):
  * P = 8192 (both kernels park the terminal values in LDS) and P = 65,536 (both replay), hardware and portable
    math: each pair warmed up, then the kernel's own execution time of --calls calls of each, alternating call by
    call (smc_time_launches: each call alone on a drained stream; medians; ratio = Greeks / price);
  * P = 8192 with SMC_PRICE_REPLAY on both calls: the forced-replay times, and each kernel's replay / lds ratio.
The two calls' common columns (prices, their standard errors, the terminal sum) are checked to agree bit for
bit before anything is timed."""

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


def window(cd: torch.Tensor, P: int, math: str, replay: bool, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = (_lib.MATH_HW if math == "hw" else 0) | (_lib.PRICE_REPLAY if replay else 0)
    greeks = torch.empty((B, _lib.GREEKS_COLS), dtype=torch.float64, device=cd.device)
    prices = torch.empty((B, _lib.PRICE_COLS), dtype=torch.float64, device=cd.device)

    def call_greeks() -> None:
        _lib.check(L.smc_gbm_greeks(_lib.ptr(cd), B, T, P, 7, None, 0, flag, _lib.NORM_NORMALIZE, _lib.DTYPE_F32,
                                    _lib.ptr(greeks), _lib.stream_handle()))

    def call_price() -> None:
        _lib.check(L.smc_gbm_price(_lib.ptr(cd), B, T, P, 7, None, 0, flag, _lib.NORM_NORMALIZE, _lib.DTYPE_F32,
                                   _lib.ptr(prices), _lib.stream_handle()))

    for _ in range(warmup):
        call_greeks()
        call_price()
    torch.cuda.synchronize()
    assert torch.equal(greeks[:, 20:25], prices[:, [0, 1, 3, 4, 7]]), "the two calls' common columns differ"
    kg, kp = [], []
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        kg += kernel_ms(call_greeks, 1)
        kp += kernel_ms(call_price, 1)

    def stats(name: str, k: list[float]) -> dict:
        return {"kernel": name, "kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
                "kernel_ms_max": round(max(k), 4)}

    return {"window": "smc_gbm_greeks beside smc_gbm_price", "B": B, "T": T, "P": P, "dtype": "float32", "math": math,
            "forced_replay": replay, "calls_each": calls,
            "greeks": stats(L.smc_gbm_greeks_kernel(T, P, flag, _lib.NORM_NORMALIZE, _lib.DTYPE_F32).decode(), kg),
            "price": stats(L.smc_gbm_price_kernel(T, P, flag, _lib.NORM_NORMALIZE, _lib.DTYPE_F32).decode(), kp),
            "ratio_greeks_to_price": round(statistics.median(kg) / statistics.median(kp), 3)}


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
    record: dict = {"tool": "tools/greeks_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION}
    windows = []
    for P in (8192, 65536):
        for math in ("hw", "portable"):
            windows.append(window(cd, P, math, False, args.calls, args.warmup))
    for math in ("hw", "portable"):
        forced = window(cd, 8192, math, True, args.calls, args.warmup)
        parked = next(w for w in windows if w["P"] == 8192 and w["math"] == math)
        for key in ("greeks", "price"):
            forced[f"{key}_replay_over_lds"] = round(forced[key]["kernel_ms_median"] / parked[key]["kernel_ms_median"], 3)
        windows.append(forced)
    record["windows"] = windows
    out = args.out or os.path.join(ROOT, "profiles", "greeks", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
