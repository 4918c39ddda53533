"""Timing of the batched basket Greeks (smc_basket_greeks, basket_greeks_kernel) against the batched basket pricer
(smc_basket_price, basket_price_kernel, which this kernel does not change) at the same shape, math and mode.
Needs a GPU.

    python tools/basket_greeks_timing.py                 # the record: profiles/basket_greeks/timing.json
    python tools/basket_greeks_timing.py --paths 8192 --calls 3 --out /dev/null   # one shape, e.g. under a kernel trace

Windows of the record (A = 4 assets, T = 16, NORMALIZE, B = 1024 contracts; P = 8192, which parks the terminal
values in LDS, and P = 131,072, C5's path count, which replays; hardware and portable math), all in one process: the
kernel's own execution time of each of --calls calls (smc_time_launches: each call alone on a drained stream; median,
min, max) of smc_basket_greeks alternating call by call with smc_basket_price, and at P = 8192 the same pair with
SMC_PRICE_REPLAY beside the default (the choice changes no output bit, which the run checks).  The run also checks
that the Greeks' price columns are the price call's bit for bit.  No time is asserted anywhere."""

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
from tools.basket_price_timing import contracts, summary  # noqa: E402
from tools.price_batch_timing import kernel_ms  # noqa: E402

A, T = 4, 16
N_COLS = 4 * A + 6


def window(cd: torch.Tensor, P: int, math: str, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    modes = (0, _lib.PRICE_REPLAY)
    greeks = {f: torch.empty((B, _lib.basket_greeks_cols(A)), dtype=torch.float64, device=cd.device) for f in modes}
    prices = {f: torch.empty((B, _lib.BASKET_PRICE_COLS), dtype=torch.float64, device=cd.device) for f in modes}
    sums = torch.empty((B, 3, A), dtype=torch.float64, device=cd.device)

    def run_greeks(f: int) -> None:
        _lib.check(L.smc_basket_greeks(_lib.ptr(cd), B, A, T, P, 7, None, 0, flag | f, _lib.NORM_NORMALIZE,
                                       _lib.ptr(greeks[f]), _lib.ptr(sums), _lib.stream_handle()))

    def run_price(f: int) -> None:
        _lib.check(L.smc_basket_price(_lib.ptr(cd), B, A, T, P, 7, None, 0, flag | f, _lib.NORM_NORMALIZE,
                                      _lib.ptr(prices[f]), None, _lib.stream_handle()))

    names = {f: (L.smc_basket_greeks_kernel(A, T, P, flag | f, _lib.NORM_NORMALIZE).decode(),
                 L.smc_basket_price_kernel(A, T, P, flag | f, _lib.NORM_NORMALIZE).decode()) for f in modes}
    flags = modes if names[0][0].endswith("(lds)") else (0,)
    for _ in range(warmup):
        for f in flags:
            run_greeks(f)
            run_price(f)
    torch.cuda.synchronize()
    for f in flags:
        assert torch.equal(greeks[f], greeks[0]), "the modes' outputs differ"
        assert torch.equal(greeks[f][:, 2 * N_COLS:], prices[f][:, [0, 1, 6, 7]]), "the price columns differ"
    times: dict[str, list[float]] = {f"{k}{f}": [] for f in flags for k in ("greeks", "price")}
    for _ in range(calls):  # alternating: drift of the clocks lands on all of them
        for f in flags:
            times[f"greeks{f}"] += kernel_ms(lambda f=f: run_greeks(f), 1)
            times[f"price{f}"] += kernel_ms(lambda f=f: run_price(f), 1)
    torch.cuda.synchronize()
    row: dict = {"A": A, "T": T, "B": B, "P": P, "math": math, "calls_each": calls}
    for f in flags:
        key = "forced_replay" if f else "default"
        g, p = statistics.median(times[f"greeks{f}"]), statistics.median(times[f"price{f}"])
        row[key] = {"greeks": {"kernel": names[f][0], **summary(times[f"greeks{f}"])},
                    "price": {"kernel": names[f][1], **summary(times[f"price{f}"])},
                    "greeks_over_price": round(g / p, 4)}
    return row


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contracts", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per window (at least 10 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", type=str, default="8192,131072")
    ap.add_argument("--maths", type=str, default="hw,portable")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    _lib.require_device()
    cd = torch.tensor(contracts(args.contracts), dtype=torch.float64, device="cuda")
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/basket_greeks_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION, "windows": []}
    for P in (int(p) for p in args.paths.split(",")):
        for math in args.maths.split(","):
            record["windows"].append(window(cd, P, math, args.calls, args.warmup))
    out = args.out or os.path.join(ROOT, "profiles", "basket_greeks", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
