"""Timing of the path-dependent batched pricer (BlackScholes.price_paths_batch_device, path_price_kernel) against
(a) the European batched pricer replaying its simulation (smc_gbm_price with SMC_PRICE_REPLAY: the same two
simulations per contract, terminal row only) and (b) the route without the fused kernel: one contract at a
time, the stored [T][P] matrix of BlackScholes._simulate reduced with torch.  Needs a GPU.

    python tools/path_price_timing.py                 # the record: profiles/path_price/timing.json

Windows of the record (T = 16, float32, NORMALIZE, B = 4096 contracts, barriers one volatility-time unit either
side of the spot / forward), all in one process:
  * price_paths_batch_device at P = 65,536 and P = 8192, hardware and portable math: each shape warmed up, then
    device events around --calls calls (ms per call, contracts/s), and the kernel's own execution time of each
    of --calls further calls (smc_time_launches: each call alone on a drained stream; the median);
  * smc_gbm_price | SMC_PRICE_REPLAY at the same shapes, the kernel's own execution time alternating call by call
    with the path pricer's (ratio = path / European, medians);
  * a loop over --loop-contracts of the same contracts at each P: _simulate, then torch reductions for the same
    eight payoffs, their means brought to the host (ms per contract, wall time)."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectralmc_amd import _lib  # noqa: E402
from spectralmc_amd.gbm import BlackScholes  # noqa: E402
from tests.helpers import expect_success  # noqa: E402
from tools.price_batch_timing import T, contracts, engine, events_ms, kernel_ms  # noqa: E402


def barriers(c: np.ndarray) -> np.ndarray:
    X0, Tm, v = c[:, 0], c[:, 2], c[:, 5]
    F = X0 * np.exp((c[:, 3] - c[:, 4]) * Tm)
    return np.stack([X0 * np.exp(-v * np.sqrt(Tm)), np.maximum(X0, F) * np.exp(v * np.sqrt(Tm))], axis=1)


def batch_window(cd: torch.Tensor, bd: torch.Tensor, P: int, math: str, calls: int, warmup: int) -> dict:
    bs = engine(P, math)
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    european = torch.empty((B, _lib.PRICE_COLS), dtype=torch.float64, device=cd.device)

    def call() -> None:
        expect_success(bs.price_paths_batch_device(cd, bd))

    def call_european() -> None:
        _lib.check(L.smc_gbm_price(_lib.ptr(cd), B, T, P, 7, None, 0, flag | _lib.PRICE_REPLAY, _lib.NORM_NORMALIZE,
                                   _lib.DTYPE_F32, _lib.ptr(european), _lib.stream_handle()))

    for _ in range(warmup):
        call()
        call_european()
    torch.cuda.synchronize()
    ms = events_ms(call, calls)
    k, ke = [], []
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        k += kernel_ms(call, 1)
        ke += kernel_ms(call_european, 1)
    return {"window": "price_paths_batch_device", "B": B, "T": T, "P": P, "dtype": "float32", "math": math,
            "kernel": L.smc_gbm_price_paths_kernel(T, P, flag, _lib.NORM_NORMALIZE, _lib.DTYPE_F32).decode(),
            "calls": calls, "ms_per_call": round(ms, 4), "contracts_per_s": round(B / ms * 1e3, 1),
            "kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
            "kernel_ms_max": round(max(k), 4),
            "european_replay": {"kernel": L.smc_gbm_price_kernel(T, P, flag | _lib.PRICE_REPLAY, _lib.NORM_NORMALIZE,
                                                                 _lib.DTYPE_F32).decode(),
                                "kernel_ms_median": round(statistics.median(ke), 4), "kernel_ms_min": round(min(ke), 4),
                                "kernel_ms_max": round(max(ke), 4)},
            "ratio_to_european_replay": round(statistics.median(k) / statistics.median(ke), 3)}


def matrix_prices(bs: BlackScholes, x: BlackScholes.Inputs, lower: float, upper: float) -> list[float]:
    """The eight payoff means of one contract from its stored path matrix."""
    sims = expect_success(bs._simulate(x)).sims
    avg, mx, mn, last = sims.mean(dim=0), sims.max(dim=0).values, sims.min(dim=0).values, sims[-1]
    alive = ~((sims <= lower) | (sims >= upper)).any(dim=0)
    df = float(np.exp(-x.r * x.T))
    put, call = torch.clamp(x.K - last, min=0), torch.clamp(last - x.K, min=0)
    pays = torch.stack([torch.clamp(x.K - avg, min=0), torch.clamp(avg - x.K, min=0), put * alive, call * alive,
                        torch.clamp(x.K - mn, min=0), torch.clamp(mx - x.K, min=0), put, call])
    return (df * pays.mean(dim=1)).tolist()  # one device-to-host copy


def loop_window(c: np.ndarray, bars: np.ndarray, P: int, n: int, warmup: int) -> dict:
    bs = engine(P)
    inputs = [BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5]) for r in c[:n].tolist()]
    for x, (lo, up) in list(zip(inputs, bars.tolist()))[:warmup]:
        matrix_prices(bs, x, lo, up)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x, (lo, up) in zip(inputs, bars.tolist()):
        matrix_prices(bs, x, lo, up)  # ends in a host copy: wall time is the call's time
    dt = time.perf_counter() - t0
    return {"window": "_simulate + torch reductions loop", "contracts": n, "T": T, "P": P, "dtype": "float32",
            "math": "portable", "ms_per_contract": round(dt / n * 1e3, 4), "contracts_per_s": round(n / dt, 1)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contracts", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per window (at least 10 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-contracts", type=int, default=64)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    _lib.require_device()
    c = contracts(args.contracts)
    bars = barriers(c)
    cd = torch.tensor(c, dtype=torch.float64, device="cuda")
    bd = torch.tensor(bars, dtype=torch.float64, device="cuda")
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/path_price_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION}
    windows = []
    for P in (65536, 8192):
        for math in ("hw", "portable"):
            windows.append(batch_window(cd, bd, P, math, args.calls, args.warmup))
        windows.append(loop_window(c, bars, P, args.loop_contracts, args.warmup))
    record["windows"] = windows
    out = args.out or os.path.join(ROOT, "profiles", "path_price", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
