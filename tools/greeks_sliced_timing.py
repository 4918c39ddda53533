"""Timing of sliced batched Greeks (smc_gbm_greeks_sliced: greeks_slice_kernel + greeks_finish_kernel, a contract cut
into slices of one workgroup each) beside the one-workgroup-per-contract call (smc_gbm_greeks, greeks_kernel) and beside
the sliced price call (smc_gbm_price_sliced) at the same shape, math and normalisation in the same process.  Needs a
GPU.

    python tools/greeks_sliced_timing.py           # the record: profiles/greeks_sliced/timing.json

Windows of the record (T = 16, the default slice length smc_gbm_price_slice_paths(P)):
  * B = 1, P = 2^24 (slice 32,768, W = 512), float32, hardware and portable math, RAW and NORMALIZE: the headline, and
    the pass mark (in each of them the sliced call has to be faster than smc_gbm_greeks in the same run);
  * B = 1, P = 65,536 (slice 2048, W = 32), float32 hw, NORMALIZE: the single quote;
  * B = 16, P = 2^20, float32 hw, NORMALIZE: a small book;
  * B = 4096, P = 65,536, float32 hw, NORMALIZE: what slicing costs where it is not needed;
  * B = 1, P = 2^20, float64, NORMALIZE: every workgroup loads the 51 KB table image of the f64 path math.
Each triple is warmed up, then timed over --calls calls of each, alternating call by call (smc_time_launches: from the
start of the call's first kernel to the end of its last, each call alone on a drained stream; medians with min/max;
speedup = unsliced / sliced; greeks_over_price = sliced Greeks / sliced price, the yardstick for what the Greeks add,
beside the unsliced greeks_kernel(replay) / price_kernel(replay) ratios of the README: 1.18 hw, 1.07 portable).  Before
any timing: with one slice the sliced call is checked to give smc_gbm_greeks | SMC_PRICE_REPLAY's block bit for bit, and
at every timed shape both Greeks blocks are checked to be finite and the sliced block's price columns to be the sliced
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
from tools.price_batch_timing import T, contracts, kernel_ms  # noqa: E402

UNSLICED_GREEKS_OVER_PRICE = {"hw": 1.18, "portable": 1.07}  # README, Greeks table (P = 65,536, replay)


def _flag(math: str) -> int:
    return _lib.MATH_HW if math == "hw" else 0


def _calls(cd: torch.Tensor, P: int, span: int, math: str, norm: int, dtype: int):
    L = _lib.lib()
    B = int(cd.shape[0])
    need = int(L.smc_gbm_greeks_sliced_workspace_bytes(B, P, span))
    pneed = int(L.smc_gbm_price_sliced_workspace_bytes(B, P, span))
    assert need > 0 and pneed > 0
    ws = torch.empty(need // 8, dtype=torch.float64, device=cd.device)
    pws = torch.empty(pneed // 8, dtype=torch.float64, device=cd.device)
    sliced = torch.full((B, _lib.GREEKS_COLS), float("nan"), dtype=torch.float64, device=cd.device)
    whole = torch.full((B, _lib.GREEKS_COLS), float("nan"), dtype=torch.float64, device=cd.device)
    price = torch.full((B, _lib.PRICE_COLS), float("nan"), dtype=torch.float64, device=cd.device)

    def call_sliced() -> None:
        _lib.check(L.smc_gbm_greeks_sliced(_lib.ptr(cd), B, T, P, span, 7, None, 0, _flag(math), norm, dtype,
                                           _lib.ptr(sliced), _lib.ptr(ws), need, _lib.stream_handle()))

    def call_whole(extra: int = 0) -> None:
        _lib.check(L.smc_gbm_greeks(_lib.ptr(cd), B, T, P, 7, None, 0, _flag(math) | extra, norm, dtype,
                                    _lib.ptr(whole), _lib.stream_handle()))

    def call_price() -> None:
        _lib.check(L.smc_gbm_price_sliced(_lib.ptr(cd), B, T, P, span, 7, None, 0, _flag(math), norm, dtype,
                                          _lib.ptr(price), _lib.ptr(pws), pneed, _lib.stream_handle()))

    return call_sliced, call_whole, call_price, sliced, whole, price


def one_slice_check(cd: torch.Tensor) -> None:
    """W = 1: the sliced call is smc_gbm_greeks | SMC_PRICE_REPLAY bit for bit."""
    for math, dtype in (("hw", _lib.DTYPE_F32), ("portable", _lib.DTYPE_F32), ("portable", _lib.DTYPE_F64)):
        for norm in (_lib.NORM_RAW, _lib.NORM_NORMALIZE):
            for P, span in ((4096, 4096), (693, 2048)):
                call_sliced, call_whole, _, sliced, whole, _ = _calls(cd[:12], P, span, math, norm, dtype)
                call_sliced()
                call_whole(_lib.PRICE_REPLAY)
                torch.cuda.synchronize()
                assert bool(torch.isfinite(whole).all()) and torch.equal(sliced, whole), \
                    ("one slice differs from smc_gbm_greeks | SMC_PRICE_REPLAY", math, dtype, norm, P)


def window(cd: torch.Tensor, P: int, math: str, norm: int, dtype: int, purpose: str, calls: int, warmup: int) -> dict:
    L = _lib.lib()
    B = int(cd.shape[0])
    span = int(L.smc_gbm_price_slice_paths(P))
    W = -(-P // span)
    call_sliced, call_whole, call_price, sliced, whole, price = _calls(cd, P, span, math, norm, dtype)
    for _ in range(warmup):
        call_sliced()
        call_whole()
        call_price()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(sliced).all()) and bool(torch.isfinite(whole).all()), "non-finite Greeks"
    assert torch.equal(sliced[:, 20:25], price[:, [0, 1, 3, 4, 7]]), "columns 20..24 are not the sliced price call's"
    scale = whole[:, :10].abs() + whole[:, 10:20]
    dev = float(((sliced[:, :10] - whole[:, :10]).abs() / scale.clamp_min(1e-300)).max())
    ks, kw, kp = [], [], []
    for _ in range(calls):  # alternating: drift of the clocks lands on all three
        ks += kernel_ms(call_sliced, 1)
        kw += kernel_ms(call_whole, 1)
        kp += kernel_ms(call_price, 1)

    def stats(name: str, k: list[float]) -> dict:
        return {"kernel": name, "kernel_ms_median": round(statistics.median(k), 4), "kernel_ms_min": round(min(k), 4),
                "kernel_ms_max": round(max(k), 4)}

    row = {"window": "smc_gbm_greeks_sliced beside smc_gbm_greeks and smc_gbm_price_sliced", "purpose": purpose, "B": B,
           "T": T, "P": P, "slice_paths": span, "slices": W, "workgroups": B * W,
           "dtype": "float64" if dtype == _lib.DTYPE_F64 else "float32", "math": math,
           "normalization": "NORMALIZE" if norm else "RAW", "calls_each": calls,
           "launches_per_sliced_call": 4 if norm else 2,
           "sliced": stats(L.smc_gbm_greeks_sliced_kernel(T, P, span, _flag(math), norm, dtype).decode(), ks),
           "unsliced": stats(L.smc_gbm_greeks_kernel(T, P, _flag(math), norm, dtype).decode(), kw),
           "price_sliced": stats(L.smc_gbm_price_sliced_kernel(T, P, span, _flag(math), norm, dtype).decode(), kp),
           "speedup_unsliced_over_sliced": round(statistics.median(kw) / statistics.median(ks), 2),
           "greeks_over_price_sliced": round(statistics.median(ks) / statistics.median(kp), 3),
           "sliced_faster_than_unsliced": statistics.median(ks) < statistics.median(kw),
           "max_difference_of_means_over_scale": dev}
    if dtype == _lib.DTYPE_F32:
        row["greeks_over_price_unsliced_readme"] = UNSLICED_GREEKS_OVER_PRICE[math]
    return row


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per call and window (at least 10 for the record)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    _lib.require_device()
    c = torch.tensor(contracts(4096), dtype=torch.float64, device="cuda")
    props = torch.cuda.get_device_properties(0)
    record: dict = {"tool": "tools/greeks_sliced_timing.py", "device": props.name, "cus": props.multi_processor_count,
                    "library": os.path.basename(_lib.LIB_PATH), "abi": _lib.ABI_VERSION,
                    "slice_rule": "smc_gbm_price_slice_paths: 2048 max(1, ceil(P / (2048 * 512)))"}
    one_slice_check(c)
    record["one_slice_bit_identical"] = True
    f32, f64, norm, raw = _lib.DTYPE_F32, _lib.DTYPE_F64, _lib.NORM_NORMALIZE, _lib.NORM_RAW
    windows = []
    for math in ("hw", "portable"):
        for n in (raw, norm):
            windows.append(window(c[:1], 1 << 24, math, n, f32, "the headline", args.calls, args.warmup))
    record["pass_mark_sliced_faster_in_every_headline_window"] = all(w["sliced_faster_than_unsliced"] for w in windows)
    windows.append(window(c[:1], 65536, "hw", norm, f32, "the single quote", args.calls, args.warmup))
    windows.append(window(c[:16], 1 << 20, "hw", norm, f32, "a small book", args.calls, args.warmup))
    windows.append(window(c, 65536, "hw", norm, f32, "what slicing costs where it is not needed", args.calls,
                          args.warmup))
    windows.append(window(c[:1], 1 << 20, "portable", norm, f64, "every workgroup loads the f64 table image",
                          args.calls, args.warmup))
    record["windows"] = windows
    out = args.out or os.path.join(ROOT, "profiles", "greeks_sliced", "timing.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    line = json.dumps(record)
    with open(out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    assert record["pass_mark_sliced_faster_in_every_headline_window"], "the sliced call is not faster at B = 1, P = 2^24"


if __name__ == "__main__":
    main()
