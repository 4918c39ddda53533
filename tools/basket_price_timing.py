"""Timing of the batched basket pricer (smc_basket_price, basket_price_kernel) against the training engine's
launch at the same shape and against the route without the fused kernel.  Needs a GPU.

    python tools/basket_price_timing.py                 # the record: profiles/basket_price/timing.json
    python tools/basket_price_timing.py --paths 8192 --calls 3 --out /dev/null   # one shape, e.g. under a kernel trace

Windows of the record (A = 4 assets, T = 16, NORMALIZE, B = 1024 contracts; P = 8192, which parks the terminal
values in LDS, and P = 131,072, C5's path count, which replays; hardware and portable math), all in one process:
  * smc_basket_price: the kernel's own execution time of each of --calls calls (smc_time_launches: each call
    alone on a drained stream; median, min, max), and at P = 8192 the same with SMC_PRICE_REPLAY, alternating
    call by call with the default (the choice changes no output bit, which the run checks);
  * smc_basket_train_targets at the same shape and math, SMC_STORE_TERMINAL, no sync area, terminal sums kept:
    basket_kernel (simulate, store the terminal rows, terminal sums) followed by basket_cf_kernel, timed the
    same way.  smc_time_launches spans the call's kernels from the first one's start to the last one's end, so
    this figure holds the CF pass as well (it re-reads the A x P terminal values of each contract once);
  * the matrix route: that call plus torch reductions of the [B][A][P] terminal rows for the six payoffs
    (device events around --calls repetitions, ms per repetition)."""

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
from tools.price_batch_timing import events_ms, kernel_ms  # noqa: E402

A, T, N = 4, 16, 256


def contracts(n: int) -> np.ndarray:
    """[n, 3A + 4] rows K, T, r, rho, X0.., d.., v.. (the contracts of tests/test_gpu_basket_price.py)."""
    rng = np.random.default_rng(2026 + A)
    rows = []
    for _ in range(n):
        x0 = rng.uniform(50, 150, A)
        k = x0.mean() * rng.uniform(0.8, 1.25)
        t, r, rho = rng.uniform(0.25, 2), rng.uniform(-0.02, 0.08), rng.uniform(-0.1, 0.8)
        rows.append([k, t, r, rho, *x0, *rng.uniform(0, 0.04, A), *rng.uniform(0.1, 0.6, A)])
    return np.array(rows, dtype=np.float64)


def summary(ms: list[float]) -> dict:
    return {"kernel_ms_median": round(statistics.median(ms), 4), "kernel_ms_min": round(min(ms), 4),
            "kernel_ms_max": round(max(ms), 4)}


def window(cd: torch.Tensor, P: int, math: str, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    flag = _lib.MATH_HW if math == "hw" else 0
    blocks = {f: torch.empty((B, _lib.BASKET_PRICE_COLS), dtype=torch.float64, device=cd.device)
              for f in (0, _lib.PRICE_REPLAY)}
    rows = torch.empty((B, A, P), dtype=torch.float32, device=cd.device)
    tsum = torch.empty((B, A), dtype=torch.float64, device=cd.device)
    targets = torch.empty((B, N), dtype=torch.complex64, device=cd.device)

    def price(f: int) -> None:
        _lib.check(L.smc_basket_price(_lib.ptr(cd), B, A, T, P, 7, None, 0, flag | f, _lib.NORM_NORMALIZE,
                                      _lib.ptr(blocks[f]), None, _lib.stream_handle()))

    def train() -> None:
        _lib.check(L.smc_basket_train_targets(_lib.ptr(cd), B, A, T, N, P // N, 7, None, 0, flag, _lib.NORM_NORMALIZE,
                                              _lib.STORE_TERMINAL, _lib.ptr(rows), 0, B, _lib.ptr(tsum),
                                              _lib.ptr(targets), None, 0, _lib.stream_handle()))

    K, Tm, r = cd[:, 0], cd[:, 1], cd[:, 2]
    F = (cd[:, 4:4 + A] * torch.exp((r[:, None] - cd[:, 4 + A:4 + 2 * A]) * Tm[:, None])).float()
    df, Kc = torch.exp(-r * Tm).float()[:, None], K.float()[:, None]

    def matrix_route() -> torch.Tensor:
        train()
        xs = rows * (F / (tsum / P).float())[:, :, None]
        under = (xs.mean(dim=1), xs.amax(dim=1), xs.amin(dim=1))
        pays = [df * torch.relu(sign * (Kc - u)) for u in under for sign in (1.0, -1.0)]
        return torch.stack([p.double().mean(dim=1) for p in pays], dim=1)

    default_name = L.smc_basket_price_kernel(A, T, P, flag, _lib.NORM_NORMALIZE).decode()
    flags = (0, _lib.PRICE_REPLAY) if default_name.endswith("(lds)") else (0,)
    for _ in range(warmup):
        for f in flags:
            price(f)
        matrix = matrix_route()
    torch.cuda.synchronize()
    if len(flags) == 2:
        assert torch.equal(blocks[0], blocks[_lib.PRICE_REPLAY]), "the modes' outputs differ"
    rel = float(((matrix - blocks[0][:, :6]).norm(dim=0) / blocks[0][:, :6].norm(dim=0)).max())
    times: dict[str, list[float]] = {"train": [], **{f"price{f}": [] for f in flags}}
    for _ in range(calls):  # alternating: drift of the clocks lands on all of them
        for f in flags:
            times[f"price{f}"] += kernel_ms(lambda f=f: price(f), 1)
        times["train"] += kernel_ms(train, 1)
    route_ms = events_ms(matrix_route, calls)
    torch.cuda.synchronize()
    sim = statistics.median(times["train"])
    row = {"A": A, "T": T, "B": B, "P": P, "math": math, "calls_each": calls,
           "price": {"kernel": default_name, **summary(times["price0"])},
           "train_targets": {"kernel": L.smc_basket_train_targets_kernel(A, T, N, P // N, 0, 1).decode(),
                             **summary(times["train"])},
           "price_over_train": round(statistics.median(times["price0"]) / sim, 4),
           "matrix_route_ms": round(route_ms, 4), "matrix_route_max_rel_diff": float(f"{rel:.3e}")}
    if len(flags) == 2:
        k = f"price{_lib.PRICE_REPLAY}"
        row["price_forced_replay"] = {"kernel": "basket_price_kernel(replay)", **summary(times[k])}
        row["forced_replay_over_train"] = round(statistics.median(times[k]) / sim, 4)
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
    record: dict = {"tool": "tools/basket_price_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION, "windows": []}
    for P in (int(p) for p in args.paths.split(",")):
        for math in args.maths.split(","):
            record["windows"].append(window(cd, P, math, args.calls, args.warmup))
    out = args.out or os.path.join(ROOT, "profiles", "basket_price", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
