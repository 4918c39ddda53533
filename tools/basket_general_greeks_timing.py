"""Timing of the Greeks of the weighted, general-correlation basket (smc_basket_greeks_general,
basket_greeks_general_kernel) against the equal-weight basket Greeks (smc_basket_greeks, basket_greeks_kernel, which
this kernel does not change) at the same shape, math and mode.  Needs a GPU.

    python tools/basket_general_greeks_timing.py         # the record: profiles/basket_general_greeks/timing.json
    python tools/basket_general_greeks_timing.py --paths 8192 --calls 3 --out /dev/null   # one shape

Windows of the record (A = 4 assets, T = 16, NORMALIZE, B = 1024 contracts; P = 8192, which parks the terminal
values in LDS, and P = 131,072, which replays; hardware and portable math), all in one process: the kernel's own
execution time of each of --calls calls (smc_time_launches: each call alone on a drained stream; median, min, max) of
smc_basket_greeks_general alternating call by call with smc_basket_greeks.  The general call takes a row of weights
and a packed correlation triangle per contract (Dirichlet weights; the row's rho moved by up to 0.05 per pair).  The
record holds the ratio of the medians and, beside it, the spread of the baseline calls ((max - min) / median).  The run
also checks that with no tables the general call's delta, vega, rho and theta columns are the baseline's bit for bit
(A = 4: f32(1 / A) is a power of two).  No time is asserted anywhere."""

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
from tools.basket_price_timing import contracts, summary  # noqa: E402
from tools.price_batch_timing import kernel_ms  # noqa: E402

A, T = 4, 16
NPAIRS = A * (A - 1) // 2


def tables(rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(weights [B, A], packed correlation [B, np]) of the general call."""
    rng = np.random.default_rng(2031)
    B = rows.shape[0]
    w = rng.dirichlet(np.ones(A), B)
    tri = rows[:, 3:4] + rng.uniform(-0.05, 0.05, (B, NPAIRS))
    return w, tri


def window(cd: torch.Tensor, wd: torch.Tensor, td: torch.Tensor, P: int, math: str, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    general = torch.empty((B, _lib.basket_greeks_general_cols(A)), dtype=torch.float64, device=cd.device)
    plain = torch.empty((B, _lib.basket_greeks_general_cols(A)), dtype=torch.float64, device=cd.device)
    base = torch.empty((B, _lib.basket_greeks_cols(A)), dtype=torch.float64, device=cd.device)
    gsums = torch.empty((B, A + A * (A + 1) // 2), dtype=torch.float64, device=cd.device)
    sums = torch.empty((B, 3, A), dtype=torch.float64, device=cd.device)

    def run_general(out=general, w=wd, t=td) -> None:
        _lib.check(L.smc_basket_greeks_general(_lib.ptr(cd), _lib.ptr(w), A if w is not None else 0, _lib.ptr(t),
                                               NPAIRS if t is not None else 0, B, A, T, P, 7, None, 0, flag,
                                               _lib.NORM_NORMALIZE, _lib.ptr(out), _lib.ptr(gsums), _lib.stream_handle()))

    def run_base() -> None:
        _lib.check(L.smc_basket_greeks(_lib.ptr(cd), B, A, T, P, 7, None, 0, flag, _lib.NORM_NORMALIZE, _lib.ptr(base),
                                       _lib.ptr(sums), _lib.stream_handle()))

    names = (L.smc_basket_greeks_general_kernel(A, T, P, flag, _lib.NORM_NORMALIZE).decode(),
             L.smc_basket_greeks_kernel(A, T, P, flag, _lib.NORM_NORMALIZE).decode())
    for _ in range(warmup):
        run_general()
        run_base()
    run_general(plain, None, None)
    torch.cuda.synchronize()
    n, m = 4 * A + 4 + 2 * NPAIRS, 4 * A + 6
    assert torch.equal(plain[:, :4 * A + 4], base[:, :4 * A + 4]), "the shared columns differ"
    assert torch.equal(plain[:, 2 * n:], base[:, 2 * m:]), "the price columns differ"
    assert bool(torch.isfinite(general).all()), "non-finite output"
    times: dict[str, list[float]] = {"general": [], "base": []}
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        times["general"] += kernel_ms(run_general, 1)
        times["base"] += kernel_ms(run_base, 1)
    torch.cuda.synchronize()
    g, b = statistics.median(times["general"]), statistics.median(times["base"])
    return {"A": A, "T": T, "B": B, "P": P, "math": math, "calls_each": calls,
            "general": {"kernel": names[0], **summary(times["general"])},
            "greeks": {"kernel": names[1], **summary(times["base"])},
            "general_over_greeks": round(g / b, 4),
            "greeks_spread": round((max(times["base"]) - min(times["base"])) / b, 4)}


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
    rows = contracts(args.contracts)
    w, tri = tables(rows)
    cd, wd, td = (torch.tensor(a, dtype=torch.float64, device="cuda") for a in (rows, w, tri))
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/basket_general_greeks_timing.py", "device": props.name,
                    "cus": props.multi_processor_count, "library": os.path.basename(_lib.LIB_PATH),
                    "abi": _lib.ABI_VERSION, "windows": []}
    for P in (int(p) for p in args.paths.split(",")):
        for math in args.maths.split(","):
            record["windows"].append(window(cd, wd, td, P, math, args.calls, args.warmup))
    out = args.out or os.path.join(ROOT, "profiles", "basket_general_greeks", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
