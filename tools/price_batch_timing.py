"""Timing of the batched Monte-Carlo pricer (BlackScholes.price_batch_device, price_kernel) against the
one-contract-at-a-time path (BlackScholes.price_to_host).  Needs a GPU.

    python tools/price_batch_timing.py                 # the record: profiles/price_batch/timing.json
    python tools/price_batch_timing.py --modes 8192,16384,32768   # lds against replay, alternating

Windows of the record (T = 16, float32, NORMALIZE, B = 4096 contracts):
  * price_batch_device at P = 65,536 and P = 8192, hardware and portable math: each shape warmed up, then
    device events around --calls calls (ms per call, contracts/s), and the kernel's own execution time of
    each of --calls further calls (smc_time_launches: each call alone on a drained stream; the median);
  * a loop of price_to_host over --loop-contracts of the same contracts at each P (unchanged by the batched
    pricer: smc_gbm_simulate + smc_gbm_normalize + torch ops + five host syncs per contract).
--modes times smc_gbm_price with and without SMC_PRICE_REPLAY at the given path counts, alternating the two
in one process (the choice changes no output bit, which the run checks).  A path count the library would
replay anyway needs a library built with a larger SMC_PRICE_PARK_BYTES (SMC_LIB_PATH selects it)."""

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
from spectralmc_amd.models.numerical import Precision  # noqa: E402
from tests.helpers import expect_success, make_black_scholes_config, make_simulation_params  # noqa: E402

T, N = 16, 256


def contracts(n: int) -> np.ndarray:
    rng = np.random.default_rng(2026)
    x0 = rng.uniform(50, 150, n)
    return np.stack([x0, x0 * rng.uniform(0.8, 1.25, n), rng.uniform(0.25, 2, n), rng.uniform(-0.02, 0.08, n),
                     rng.uniform(0, 0.04, n), rng.uniform(0.1, 0.6, n)], axis=1)


def engine(P: int, math: str = "portable") -> BlackScholes:
    sp = make_simulation_params(timesteps=T, network_size=N, batches_per_mc_run=P // N, mc_seed=7, buffer_size=1,
                                dtype=Precision.float32)
    bs = BlackScholes(make_black_scholes_config(sim_params=sp))
    bs.price_batch_math = math
    return bs


def events_ms(fn, calls: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def kernel_ms(fn, calls: int) -> list[float]:
    """The kernel's own execution time of each call, alone on a drained stream (smc_time_launches)."""
    L = _lib.lib()
    out = []
    for _ in range(calls):
        k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k0.record()
        k1.record()
        torch.cuda.synchronize()
        _lib.check(L.smc_time_launches(k0.cuda_event, k1.cuda_event))
        try:
            fn()
        finally:
            _lib.check(L.smc_time_launches(None, None))
        torch.cuda.synchronize()
        out.append(k0.elapsed_time(k1))
    return out


def batch_window(cd: torch.Tensor, P: int, math: str, calls: int, warmup: int) -> dict:
    bs = engine(P, math)
    B = int(cd.shape[0])

    def call() -> None:
        expect_success(bs.price_batch_device(cd))

    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = events_ms(call, calls)
    k = kernel_ms(call, calls)
    name = _lib.lib().smc_gbm_price_kernel(T, P, _lib.MATH_HW if math == "hw" else 0, _lib.NORM_NORMALIZE,
                                           _lib.DTYPE_F32).decode()
    return {"window": "price_batch_device", "B": B, "T": T, "P": P, "dtype": "float32", "math": math, "kernel": name,
            "calls": calls, "ms_per_call": round(ms, 4), "contracts_per_s": round(B / ms * 1e3, 1),
            "kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
            "kernel_ms_max": round(max(k), 4)}


def loop_window(c: np.ndarray, P: int, n: int, warmup: int) -> dict:
    bs = engine(P)
    inputs = [BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5]) for r in c[:n].tolist()]
    for x in inputs[:warmup]:
        expect_success(bs.price_to_host(x))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x in inputs:
        expect_success(bs.price_to_host(x))  # ends in host syncs: wall time is the call's time
    dt = time.perf_counter() - t0
    return {"window": "price_to_host loop", "contracts": n, "T": T, "P": P, "dtype": "float32", "math": "portable",
            "ms_per_contract": round(dt / n * 1e3, 4), "contracts_per_s": round(n / dt, 1)}


def modes(cd: torch.Tensor, paths: list[int], calls: int, warmup: int) -> list[dict]:
    L = _lib.lib()
    B = int(cd.shape[0])
    out = []
    for P in paths:
        block = {f: torch.empty((B, _lib.PRICE_COLS), dtype=torch.float64, device=cd.device) for f in (0, _lib.PRICE_REPLAY)}

        def call(flag: int) -> None:
            _lib.check(L.smc_gbm_price(_lib.ptr(cd), B, T, P, 7, None, 0, flag, _lib.NORM_NORMALIZE, _lib.DTYPE_F32,
                                       _lib.ptr(block[flag]), _lib.stream_handle()))

        names = {f: L.smc_gbm_price_kernel(T, P, f, _lib.NORM_NORMALIZE, _lib.DTYPE_F32).decode() for f in block}
        for _ in range(warmup):
            for f in block:
                call(f)
        torch.cuda.synchronize()
        assert torch.equal(block[0], block[_lib.PRICE_REPLAY]), "the modes' outputs differ"
        times: dict[int, list[float]] = {f: [] for f in block}
        for _ in range(calls):  # alternating: drift of the clocks lands on both
            for f in block:
                times[f] += kernel_ms(lambda f=f: call(f), 1)
        row = {"window": "lds against replay", "B": B, "T": T, "P": P, "dtype": "float32", "math": "portable",
               "calls_each": calls}
        for f, key in ((0, "default"), (_lib.PRICE_REPLAY, "flagged")):
            row[key] = {"kernel": names[f], "kernel_ms_median": round(statistics.median(times[f]), 4),
                        "kernel_ms_min": round(min(times[f]), 4), "kernel_ms_max": round(max(times[f]), 4)}
        out.append(row)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contracts", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per window (at least 10 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-contracts", type=int, default=64)
    ap.add_argument("--modes", type=str, default="", help="comma-separated path counts: lds against replay only")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    _lib.require_device()
    c = contracts(args.contracts)
    cd = torch.tensor(c, dtype=torch.float64, device="cuda")
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/price_batch_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION}
    if args.modes:
        record["windows"] = modes(cd, [int(p) for p in args.modes.split(",")], args.calls, args.warmup)
        default_out = os.path.join(ROOT, "profiles", "price_batch", "modes.json")
    else:
        windows = []
        for P in (65536, 8192):
            for math in ("hw", "portable"):
                windows.append(batch_window(cd, P, math, args.calls, args.warmup))
            windows.append(loop_window(c, P, args.loop_contracts, args.warmup))
        record["windows"] = windows
        default_out = os.path.join(ROOT, "profiles", "price_batch", "timing.json")
    out = args.out or default_out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
