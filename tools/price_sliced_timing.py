"""Timing of sliced batched pricing (smc_gbm_price_sliced: price_slice_kernel + price_finish_kernel, a contract cut
into slices of one workgroup each) beside the one-workgroup-per-contract call (smc_gbm_price, price_kernel) at the same
shape, math and normalisation in the same process.  Needs a GPU.

    python tools/price_sliced_timing.py           # the record: profiles/price_sliced/timing.json

Windows of the record (T = 16, the default slice length smc_gbm_price_slice_paths(P)):
  * B = 1, P = 2^24 (slice 32,768, W = 512), float32, hardware and portable math, RAW and NORMALIZE: the headline;
  * B = 1, P = 65,536 (slice 2048, W = 32), float32, both maths, NORMALIZE: the single quote, and beside it the wall
    time of price_to_host for the same contract;
  * B = 16, P = 2^20, float32 hw, NORMALIZE: a small book;
  * B = 4096, P = 65,536, float32 hw, NORMALIZE: what slicing costs where it is not needed;
  * B = 1, P = 2^20, float64, NORMALIZE: every workgroup loads the 51 KB table image of the f64 path math.
Each pair is warmed up, then timed over --calls calls of each, alternating call by call (smc_time_launches: from the
start of the call's first kernel to the end of its last, each call alone on a drained stream; medians with min/max;
speedup = unsliced / sliced).  Before any timing: with one slice the sliced call is checked to give
smc_gbm_price | SMC_PRICE_REPLAY's block bit for bit, and at every timed shape both calls' blocks are checked to be
finite and to agree to 1e-6 relative in the means (the f64 sums are associated by slice, so under NORMALIZE the
float32 scale may sit one rounding apart)."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from spectralmc_amd import _lib  # noqa: E402
from spectralmc_amd.gbm import BlackScholes  # noqa: E402
from tests.helpers import expect_success  # noqa: E402
from tools.price_batch_timing import T, contracts, engine, kernel_ms  # noqa: E402

# the project's own records of price_kernel(replay) at B = 4096, P = 65,536, T = 16 (README): ms per call, hence per
# 2^24 paths of one contract at full occupancy (two simulations, NORMALIZE)
YARDSTICK_MS = {"hw": 2.924, "portable": 8.540}


def _flag(math: str) -> int:
    return _lib.MATH_HW if math == "hw" else 0


def _calls(cd: torch.Tensor, P: int, span: int, math: str, norm: int, dtype: int):
    L = _lib.lib()
    B = int(cd.shape[0])
    need = int(L.smc_gbm_price_sliced_workspace_bytes(B, P, span))
    assert need > 0
    ws = torch.empty(need // 8, dtype=torch.float64, device=cd.device)
    sliced = torch.full((B, _lib.PRICE_COLS), float("nan"), dtype=torch.float64, device=cd.device)
    whole = torch.full((B, _lib.PRICE_COLS), float("nan"), dtype=torch.float64, device=cd.device)

    def call_sliced() -> None:
        _lib.check(L.smc_gbm_price_sliced(_lib.ptr(cd), B, T, P, span, 7, None, 0, _flag(math), norm, dtype,
                                          _lib.ptr(sliced), _lib.ptr(ws), need, _lib.stream_handle()))

    def call_whole(extra: int = 0) -> None:
        _lib.check(L.smc_gbm_price(_lib.ptr(cd), B, T, P, 7, None, 0, _flag(math) | extra, norm, dtype,
                                   _lib.ptr(whole), _lib.stream_handle()))

    return call_sliced, call_whole, sliced, whole


def one_slice_check(cd: torch.Tensor) -> None:
    """W = 1: the sliced call is smc_gbm_price | SMC_PRICE_REPLAY bit for bit."""
    for math, dtype in (("hw", _lib.DTYPE_F32), ("portable", _lib.DTYPE_F32), ("portable", _lib.DTYPE_F64)):
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            for P, span in ((4096, 4096), (693, 2048)):
                call_sliced, call_whole, sliced, whole = _calls(cd[:12], P, span, math, norm, dtype)
                call_sliced()
                call_whole(_lib.PRICE_REPLAY)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(whole).all()) and torch.equal(sliced, whole), \
                    ("one slice differs from smc_gbm_price | SMC_PRICE_REPLAY", math, dtype, norm, P)


def window(cd: torch.Tensor, P: int, math: str, norm: int, dtype: int, purpose: str, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    span = int(L.smc_gbm_price_slice_paths(P))
    W = -(-P // span)
    call_sliced, call_whole, sliced, whole = _calls(cd, P, span, math, norm, dtype)
    for _ in range(warmup):
        call_sliced()
        call_whole()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sliced).all()) and bool(torch.isfinite(whole).all()), "non-finite prices"
    assert torch.equal(sliced[:, 5:7], whole[:, 5:7]), "the intrinsic values differ"
    rel = ((sliced[:, [0, 1, 2, 7]] - whole[:, [0, 1, 2, 7]]).abs() / whole[:, [0, 1, 2, 7]].abs().clamp_min(1e-300)).max()
    assert float(rel) < 1e-6, f"sliced and unsliced means differ by {float(rel):.3e} relative"
    ks, kw = [], []
    for _ in range(calls):  # alternating: drift of the clocks lands on both
        ks += kernel_ms(call_sliced, 1)
        kw += kernel_ms(call_whole, 1)

    def stats(name: str, k: list[float]) -> dict:
        return {"kernel": name, "kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
                "kernel_ms_max": round(max(k), 4)}

    row = {"window": "smc_gbm_price_sliced beside smc_gbm_price", "purpose": purpose, "B": B, "T": T, "P": P,
           "slice_paths": span, "slices": W, "workgroups": B * W,
           "dtype": "float64" if dtype == _lib.DTYPE_F64 else "float32", "math": math,
           "normalization": "NORMALIZE" if norm else "RAW", "calls_each": calls,
           "launches_per_sliced_call": 4 if norm else 2,
           "sliced": stats(L.smc_gbm_price_sliced_kernel(T, P, span, _flag(math), norm, dtype).decode(), ks),
           "unsliced": stats(L.smc_gbm_price_kernel(T, P, _flag(math), norm, dtype).decode(), kw),
           "speedup_unsliced_over_sliced": round(statistics.median(kw) / statistics.median(ks), 2),
           "max_rel_difference_of_means": float(rel)}
    if dtype == _lib.DTYPE_F32:
        # the full-occupancy yardstick for these B P paths: price_kernel(replay)'s 4096 x 65,536 record is two
        # simulations; RAW is one
        yard = YARDSTICK_MS[math] * (B * P) / (4096 * 65536) * (1.0 if norm else 0.5)
        row["yardstick_ms"] = round(yard, 4)
        row["sliced_over_yardstick"] = round(statistics.median(ks) / yard, 2)
    return row


def quote_window(P: int, n: int, warmup: int) -> dict:
    """price_to_host of the single quote's contract: wall time per call (it ends in host syncs)."""
    bs = engine(P)
    r = contracts(1)[0].tolist()
    x = BlackScholes.Inputs(X0=r[0], K=r[1], T=r[2], r=r[3], d=r[4], v=r[5])
    for _ in range(warmup):
        expect_success(bs.price_to_host(x))
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        expect_success(bs.price_to_host(x))
        times.append((time.perf_counter() - t0) * 1e3)
    return {"window": "price_to_host", "purpose": "the single quote, the path it had before", "B": 1, "T": T, "P": P,
            "dtype": "float32", "math": "portable", "normalization": "NORMALIZE", "calls": n,
            "wall_ms_median": round(statistics.median(times), 4), "wall_ms_min": round(min(times), 4),
            "wall_ms_max": round(max(times), 4)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per call and window (at least 10 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    _lib.require_device()
    c = torch.tensor(contracts(4096), dtype=torch.float64, device="cuda")
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/price_sliced_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION,
                    "slice_rule": "2048 max(1, ceil(P / (2048 * 512)))"}
    one_slice_check(c)
    record["one_slice_bit_identical"] = True
    f32, f64, norm, raw = _lib.DTYPE_F32, _lib.DTYPE_F64, _lib.NORM_NORMALIZE, _lib.NORM_RAW
    windows = []
    for math in ("hw", "portable"):
        for n in (raw, norm):
            windows.append(window(c[:1], 1 << 24, math, n, f32, "the headline", args.calls, args.warmup))
    for math in ("hw", "portable"):
        windows.append(window(c[:1], 65536, math, norm, f32, "the single quote", args.calls, args.warmup))
    windows.append(quote_window(65536, args.calls, args.warmup))
    windows.append(window(c[:16], 1 << 20, "hw", norm, f32, "a small book", args.calls, args.warmup))
    windows.append(window(c, 65536, "hw", norm, f32, "what slicing costs where it is not needed", args.calls,
                          args.warmup))
    windows.append(window(c[:1], 1 << 20, "portable", norm, f64, "every workgroup loads the f64 table image",
                          args.calls, args.warmup))
    record["windows"] = windows
    out = args.out or os.path.join(ROOT, "profiles", "price_sliced", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
