"""Timing of the path-dependent basket pricer (smc_basket_price_paths, basket_path_kernel) against
smc_basket_price_general | SMC_PRICE_REPLAY at the same shape in the same run.  Needs a GPU.

    python tools/basket_path_timing.py                 # the record: profiles/basket_path/timing.json
    python tools/basket_path_timing.py --paths 8192 --calls 3 --out /dev/null   # one shape

Windows of the record (A = 4 assets, T = 16, B = 1024 contracts; P = 8192 and P = 131,072; hardware and portable
math; RAW and NORMALIZE), all in one process: the kernel's own execution time of each of --calls calls of
smc_basket_price_paths (one row of Dirichlet weights, one packed correlation triangle and one row of barriers per
contract) and of the replay price call on the same tables, alternating call by call so that drift of the clocks lands
on both (smc_time_launches: each call alone on a drained stream; median, min, max).  paths_over_price is the ratio of
the medians; price_spread is (max - min) / median of the price calls themselves, the yardstick a ratio's distance from
its expectation is read against.  expected_simulations is what the pass structure alone predicts, written down before
any measurement: under RAW one simulation against the price call's one; under NORMALIZE
1 + sum of the sweeps' last rows / T against its two.  Before timing, the run checks that the European columns and the
terminal sums are the price call's bit for bit."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectralmc_amd import _lib  # noqa: E402
from tools.basket_general_timing import tables  # noqa: E402
from tools.basket_price_timing import A, T, contracts, summary  # noqa: E402
from tools.price_batch_timing import kernel_ms  # noqa: E402

LDS, SCRATCH, ROW = 144 * 1024, 2112, 512 * 8  # the header's rule for the sweep length


def expected_simulations(normalize: bool) -> dict:
    """Path simulations per call from the pass structure (A <= 4: one column group)."""
    if not normalize:
        return {"paths": 1.0, "price": 1.0, "ratio": 1.0}
    dates = min(T, (LDS - SCRATCH - (A * T * 4 + 7) // 8 * 8) // ROW // A)
    ends = [min(t0 + dates, T) for t0 in range(0, T, dates)]
    sims = 1.0 + sum(ends) / T
    return {"paths": sims, "price": 2.0, "ratio": round(sims / 2.0, 4), "sweep_dates": dates}


def barriers(rows: np.ndarray, w: np.ndarray) -> np.ndarray:
    """[n, 3]: the basket knocked out 25 % below and 35 % above its forward, the worst asset at half its lowest forward."""
    F = rows[:, 4:4 + A] * np.exp((rows[:, 2:3] - rows[:, 4 + A:4 + 2 * A]) * rows[:, 1:2])
    Fb = (w * F).sum(axis=1)
    return np.stack([0.75 * Fb, 1.35 * Fb, 0.5 * F.min(axis=1)], axis=1)


def window(cd, wd, td, bd, P: int, math: str, normalize: bool, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    norm = _lib.NORM_NORMALIZE if normalize else _lib.NORM_RAW
    out = torch.empty((B, _lib.BASKET_PATH_COLS), dtype=torch.float64, device=cd.device)
    ref = torch.empty((B, _lib.BASKET_PRICE_COLS), dtype=torch.float64, device=cd.device)
    sums = torch.empty((2, B, A), dtype=torch.float64, device=cd.device)

    def paths() -> None:
        _lib.check(L.smc_basket_price_paths(_lib.ptr(cd), _lib.ptr(wd), A, _lib.ptr(td), td.shape[1], _lib.ptr(bd), B, A,
                                            T, P, 7, None, 0, flag, norm, _lib.ptr(out), _lib.ptr(sums[0]),
                                            _lib.stream_handle()))

    def price() -> None:
        _lib.check(L.smc_basket_price_general(_lib.ptr(cd), _lib.ptr(wd), A, _lib.ptr(td), td.shape[1], B, A, T, P, 7,
                                              None, 0, flag | _lib.PRICE_REPLAY, norm, _lib.ptr(ref), _lib.ptr(sums[1]),
                                              _lib.stream_handle()))

    for _ in range(warmup):
        paths()
        price()
    torch.cuda.synchronize()
    assert torch.equal(out[:, [8, 9, 18, 19]], ref[:, [0, 1, 6, 7]]), "the European columns are not the price call's"
    assert torch.equal(sums[0], sums[1]), "the terminal sums are not the price call's"
    assert bool(torch.isfinite(out).all())
    times: dict[str, list[float]] = {"paths": [], "price": []}
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        times["paths"] += kernel_ms(paths, 1)
        times["price"] += kernel_ms(price, 1)
    torch.cuda.synchronize()
    med = statistics.median(times["price"])
    return {"A": A, "T": T, "B": B, "P": P, "math": math, "normalization": "NORMALIZE" if normalize else "RAW",
            "calls_each": calls, "knocked_share_mean": round(float(out[:, 21].mean()), 4),
            "paths": {"kernel": L.smc_basket_price_paths_kernel(A, T, P, flag, norm).decode(), **summary(times["paths"])},
            "price": {"kernel": L.smc_basket_price_general_kernel(A, T, P, flag | _lib.PRICE_REPLAY, norm).decode(),
                      **summary(times["price"])},
            "expected_simulations": expected_simulations(normalize),
            "paths_over_price": round(statistics.median(times["paths"]) / med, 4),
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
    cd, wd, td, bd = (torch.tensor(a, dtype=torch.float64, device="cuda") for a in (rows, w, tri, barriers(rows, w)))
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/basket_path_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION, "windows": []}
    for P in (int(p) for p in args.paths.split(",")):
        for math in args.maths.split(","):
            for norm in args.norms.split(","):
                record["windows"].append(window(cd, wd, td, bd, P, math, norm == "NORMALIZE", args.calls, args.warmup))
    out = args.out or os.path.join(ROOT, "profiles", "basket_path", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
