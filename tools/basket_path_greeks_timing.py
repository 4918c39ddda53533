"""Timing of the Greeks of the Asian and lookback basket options (smc_basket_greeks_paths,
basket_path_greeks_kernel) against smc_basket_price_paths (no barriers) at the same shape, math and normalisation in
the same run.  Needs a GPU.

    python tools/basket_path_greeks_timing.py                 # the record: profiles/basket_path_greeks/timing.json
    python tools/basket_path_greeks_timing.py --paths 8192 --calls 3 --out /dev/null   # one shape

Windows of the record (A = 4 assets, T = 16, B = 1024 contracts; P = 8192 and P = 131,072; hardware and portable
math; RAW and NORMALIZE), all in one process: the kernel's own execution time of each of --calls calls of
smc_basket_greeks_paths (one row of Dirichlet weights and one packed correlation triangle per contract) and of
smc_basket_price_paths on the same tables, alternating call by call so that drift of the clocks lands on both
(smc_time_launches: each call alone on a drained stream; median, min, max).  greeks_over_price is the ratio of the
medians; price_spread is (max - min) / median of the price calls themselves, the yardstick a ratio's distance from
its expectation is read against; bump_calls_over_greeks is what the 4A + 5 pricing calls of bump and revalue cost
against this one call.  expected_simulations is what the pass structure alone predicts, written down before any
measurement.  Before timing, the run checks that the four price columns and their errors are the
price call's bit for bit."""

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
from tools.basket_general_timing import tables  # noqa: E402
from tools.basket_price_timing import A, T, contracts, summary  # noqa: E402
from tools.price_batch_timing import kernel_ms  # noqa: E402

LDS, ROW = 144 * 1024, 512 * 8
PRICE_SCRATCH, GREEKS_SCRATCH = 2112, 3328  # the header's rules for the two sweep lengths


def _sweep_simulations(dates: int) -> float:
    """Simulations the NORMALIZE sweeps cost: each sweep runs from row 0 to its last row."""
    return sum(min(t0 + dates, T) for t0 in range(0, T, dates)) / T


def expected_simulations(normalize: bool) -> dict:
    """Path simulations per call from the pass structure (A <= 4: two payoff passes against the price call's one)."""
    if not normalize:
        return {"greeks": 2.0, "price": 1.0, "ratio": 2.0}
    price_dates = min(T, (LDS - PRICE_SCRATCH - (A * T * 4 + 7) // 8 * 8) // ROW // A)
    greeks_dates = min(T, (LDS - GREEKS_SCRATCH - ((3 * A + 1) * T * 4 + 7) // 8 * 8) // (2 * A * ROW))
    g, p = 2.0 + _sweep_simulations(greeks_dates), 1.0 + _sweep_simulations(price_dates)
    return {"greeks": g, "price": p, "ratio": round(g / p, 4), "greeks_sweep_dates": greeks_dates,
            "price_sweep_dates": price_dates}


def window(cd, wd, td, P: int, math: str, normalize: bool, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    norm = _lib.NORM_NORMALIZE if normalize else _lib.NORM_RAW
    G = 2 * A + 2
    out = torch.empty((B, _lib.basket_path_greeks_cols(A)), dtype=torch.float64, device=cd.device)
    ref = torch.empty((B, _lib.BASKET_PATH_COLS), dtype=torch.float64, device=cd.device)

    def greeks() -> None:
        _lib.check(L.smc_basket_greeks_paths(_lib.ptr(cd), _lib.ptr(wd), A, _lib.ptr(td), td.shape[1], B, A, T, P, 7,
                                             None, 0, flag, norm, _lib.ptr(out), _lib.stream_handle()))

    def price() -> None:
        _lib.check(L.smc_basket_price_paths(_lib.ptr(cd), _lib.ptr(wd), A, _lib.ptr(td), td.shape[1], None, B, A, T, P,
                                            7, None, 0, flag, norm, _lib.ptr(ref), None, _lib.stream_handle()))

    for _ in range(warmup):
        greeks()
        price()
    torch.cuda.synchronize()
    assert torch.equal(out[:, 8 * G:], ref[:, [0, 1, 4, 5, 10, 11, 14, 15]]), "the price columns are not the price call's"
    assert bool(torch.isfinite(out).all())
    times: dict[str, list[float]] = {"greeks": [], "price": []}
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        times["greeks"] += kernel_ms(greeks, 1)
        times["price"] += kernel_ms(price, 1)
    torch.cuda.synchronize()
    med = statistics.median(times["price"])
    ratio = statistics.median(times["greeks"]) / med
    return {"A": A, "T": T, "B": B, "P": P, "math": math, "normalization": "NORMALIZE" if normalize else "RAW",
            "calls_each": calls,
            "greeks": {"kernel": L.smc_basket_greeks_paths_kernel(A, T, P, flag, norm).decode(), **summary(times["greeks"])},
            "price": {"kernel": L.smc_basket_price_paths_kernel(A, T, P, flag, norm).decode(), **summary(times["price"])},
            "expected_simulations": expected_simulations(normalize),
            "greeks_over_price": round(ratio, 4),
            "bump_calls": 4 * A + 5, "bump_calls_over_greeks": round((4 * A + 5) / ratio, 4),
            "price_spread": round((max(times["price"]) - min(times["price"])) / med, 4)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contracts", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per window (at least 10 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--paths", type=str, default="8192,131072")
    ap.add_argument("--maths", type=str, default="hw,portable")
    ap.add_argument("--norms", type=str, default="RAW,NORMALIZE")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    _lib.require_device()
    rows = contracts(args.contracts)
    w, tri = tables(args.contracts)
    cd, wd, td = (torch.tensor(a, dtype=torch.float64, device="cuda") for a in (rows, w, tri))
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/basket_path_greeks_timing.py", "device": props.name,
                    "cus": props.multi_processor_count, "library": os.path.basename(_lib.LIB_PATH),
                    "abi": _lib.ABI_VERSION, "windows": []}
    for P in (int(p) for p in args.paths.split(",")):
        for math in args.maths.split(","):
            for norm in args.norms.split(","):
                record["windows"].append(window(cd, wd, td, P, math, norm == "NORMALIZE", args.calls, args.warmup))
    out = args.out or os.path.join(ROOT, "profiles", "basket_path_greeks", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
