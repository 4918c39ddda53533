"""Timing of the weighted, general-correlation basket pricer (smc_basket_price_general, basket_general_kernel)
against smc_basket_price at the same shape in the same run.  Needs a GPU.

    python tools/basket_general_timing.py                 # the record: profiles/basket_general/timing.json
    python tools/basket_general_timing.py --paths 8192 --calls 3 --out /dev/null   # one shape

Windows of the record (A = 4 assets, T = 16, NORMALIZE, B = 1024 contracts; P = 8192, which parks the terminal
values in LDS, and P = 131,072, which replays; hardware and portable math), all in one process: the kernel's own
execution time of each of --calls calls of smc_basket_price_general (one row of Dirichlet weights and one packed
correlation triangle per contract) and of smc_basket_price, alternating call by call so that drift of the clocks
lands on both (smc_time_launches: each call alone on a drained stream; median, min, max).  general_over_price is the
ratio of the medians; price_spread is (max - min) / median of the price calls themselves, the yardstick a ratio's
distance from 1 is read against.  Before timing, the run checks that with NULL tables the general call gives
smc_basket_price's block bit for bit (A = 4: f32(1 / A) is a power of two)."""

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
from tools.basket_price_timing import A, T, contracts, summary  # noqa: E402
from tools.price_batch_timing import kernel_ms  # noqa: E402


def tables(n: int) -> tuple[np.ndarray, np.ndarray]:
    """(weights [n, A], packed correlation triangles [n, A (A - 1) / 2]): Dirichlet(1) weights; G G^T + diag(U(0.3, 1))
    rescaled to a unit diagonal, G an A x 2 normal matrix."""
    rng = np.random.default_rng(2028 + A)
    w = rng.dirichlet(np.ones(A), n)
    tri = np.empty((n, A * (A - 1) // 2))
    for b in range(n):
        G = rng.standard_normal((A, 2))
        C = G @ G.T + np.diag(rng.uniform(0.3, 1.0, A))
        s = 1.0 / np.sqrt(np.diag(C))
        C = C * s[:, None] * s[None, :]
        tri[b] = [C[i, k] for i in range(A) for k in range(i)]
    return w, tri


def window(cd: torch.Tensor, wd: torch.Tensor, td: torch.Tensor, P: int, math: str, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    out = {k: torch.empty((B, _lib.BASKET_PRICE_COLS), dtype=torch.float64, device=cd.device)
           for k in ("price", "general", "null")}

    def price() -> None:
        _lib.check(L.smc_basket_price(_lib.ptr(cd), B, A, T, P, 7, None, 0, flag, _lib.NORM_NORMALIZE,
                                      _lib.ptr(out["price"]), None, _lib.stream_handle()))

    def general(w: torch.Tensor | None = wd, tri: torch.Tensor | None = td, key: str = "general") -> None:
        _lib.check(L.smc_basket_price_general(
            _lib.ptr(cd), _lib.ptr(w), 0 if w is None else A, _lib.ptr(tri), 0 if tri is None else td.shape[1], B, A, T,
            P, 7, None, 0, flag, _lib.NORM_NORMALIZE, _lib.ptr(out[key]), None, _lib.stream_handle()))

    for _ in range(warmup):
        price()
        general()
        general(None, None, "null")
    torch.cuda.synchronize()
    assert torch.equal(out["null"], out["price"]), "NULL tables do not give smc_basket_price's block"
    assert bool(torch.isfinite(out["general"]).all())
    times: dict[str, list[float]] = {"price": [], "general": []}
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        times["general"] += kernel_ms(general, 1)
        times["price"] += kernel_ms(price, 1)
    torch.cuda.synchronize()
    med = statistics.median(times["price"])
    return {"A": A, "T": T, "B": B, "P": P, "math": math, "calls_each": calls,
            "general": {"kernel": L.smc_basket_price_general_kernel(A, T, P, flag, _lib.NORM_NORMALIZE).decode(),
                        **summary(times["general"])},
            "price": {"kernel": L.smc_basket_price_kernel(A, T, P, flag, _lib.NORM_NORMALIZE).decode(),
                      **summary(times["price"])},
            "general_over_price": round(statistics.median(times["general"]) / med, 4),
            "price_spread": round((max(times["price"]) - min(times["price"])) / med, 4)}


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
    w, tri = tables(args.contracts)
    wd = torch.tensor(w, dtype=torch.float64, device="cuda")
    td = torch.tensor(tri, dtype=torch.float64, device="cuda")
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/basket_general_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION, "windows": []}
    for P in (int(p) for p in args.paths.split(",")):
        for math in args.maths.split(","):
            record["windows"].append(window(cd, wd, td, P, math, args.calls, args.warmup))
    out = args.out or os.path.join(ROOT, "profiles", "basket_general", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
