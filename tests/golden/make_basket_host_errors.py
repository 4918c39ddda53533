"""Record the error surface of the basket entry points of libspectralmc_hip.so into
tests/golden/basket_host_errors.json (data only): for a fixed table of rejected (or empty) calls the status code and
the full last_error text, and the ``*_kernel`` name of a grid of shapes.  tests/test_basket_host_errors.py replays the
file against the built library, so a change of the host layer that moves a check, rewords a message or shifts the
parking bound shows as a difference.  No call of the table reaches a launch: each has a rejected argument or no
contracts.  SMC_LIB_PATH selects the library that is recorded.

    SMC_LIB_PATH=/path/to/libspectralmc_hip.so python tests/golden/make_basket_host_errors.py
"""

from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from spectralmc_amd import _lib  # noqa: E402

BUF = "buf"  # a non-NULL pointer (the replaying test passes a host array that must stay untouched)
HW, REPLAY, RAW, NORM = _lib.MATH_HW, _lib.PRICE_REPLAY, _lib.NORM_RAW, _lib.NORM_NORMALIZE

# argument names in call order, and a base call that passes every check
_PLAIN = ("contracts", "B", "A", "T", "P", "seed", "ordinal", "ordinal0", "math", "norm", "out", "sums", "stream")
_GENERAL = ("contracts", "weights", "ws", "corr", "cs", "B", "A", "T", "P", "seed", "ordinal", "ordinal0", "math",
            "norm", "out", "sums", "stream")
_PATHS = _GENERAL[:5] + ("barriers",) + _GENERAL[5:]
_BASE = dict(contracts=BUF, weights=BUF, ws=4, corr=BUF, cs=6, barriers=BUF, B=1, A=4, T=16, P=1024, seed=7,
             ordinal=None, ordinal0=0, math=0, norm=NORM, out=BUF, sums=BUF, stream=None)
BATCHED = {"smc_basket_price": _PLAIN, "smc_basket_greeks": _PLAIN, "smc_basket_price_general": _GENERAL,
           "smc_basket_greeks_general": _GENERAL, "smc_basket_price_paths": _PATHS}
_TRAIN = ("contracts", "B", "A", "T", "N", "M", "seed", "ordinal", "ordinal0", "math", "norm", "store", "paths",
          "pitch", "chunk", "sums", "targets", "sync", "sync_bytes", "stream")
_TRAIN_BASE = dict(contracts=BUF, B=1, A=4, T=16, N=64, M=32, seed=7, ordinal=None, ordinal0=0, math=0, norm=NORM,
                   store=_lib.STORE_TERMINAL, paths=BUF, pitch=0, chunk=1, sums=BUF, targets=BUF, sync=None,
                   sync_bytes=0, stream=None)

BIG_T = 40000  # 4 * 40000 f32 scales do not fit the path kernel's LDS table

# one rejected argument each ...
_SINGLE = [dict(contracts=None), dict(out=None), dict(A=0), dict(A=9), dict(math=1), dict(math=0x2000),
           dict(math=HW | REPLAY | _lib.TRAIN_DYNAMIC), dict(norm=7), dict(norm=-1), dict(T=0), dict(P=0),
           dict(P=1 << 40)]
_STRIDES = [dict(ws=3), dict(ws=-1), dict(cs=5), dict(cs=-1)]
# ... and two at once: the first check in the entry's order answers
_PAIRS = [dict(contracts=None, out=None), dict(out=None, A=9), dict(A=9, math=1), dict(math=1, norm=7),
          dict(norm=7, T=0), dict(norm=7, B=-1), dict(T=0, P=1 << 40), dict(P=0, A=0), dict(B=1 << 31, P=1 << 40)]
_STRIDE_PAIRS = [dict(P=1 << 40, ws=3), dict(T=0, cs=5), dict(ws=3, cs=5), dict(A=9, ws=3), dict(B=-1, ws=3)]
_PATH_ONLY = [dict(T=BIG_T), dict(T=BIG_T, norm=RAW, B=0), dict(T=BIG_T, ws=3), dict(T=BIG_T, cs=5),
              dict(T=BIG_T, P=0), dict(T=BIG_T, A=9), dict(T=BIG_T, out=None)]
# optional pointers left NULL and strides that nobody reads: accepted, so recorded on the empty batch only
_ACCEPTED = [dict(), dict(sums=None), dict(ordinal=BUF), dict(math=HW | REPLAY, norm=RAW)]
_ACCEPTED_GENERAL = [dict(weights=None, ws=-7), dict(corr=None, cs=-7), dict(weights=None, corr=None),
                     dict(ws=0, cs=0), dict(A=1, cs=0), dict(barriers=None)]


def call_table() -> list[tuple[str, dict]]:
    """(entry, keyword arguments) of every recorded call, in a fixed order."""
    out: list[tuple[str, dict]] = []
    for entry, names in BATCHED.items():
        general = "ws" in names
        rejected = _SINGLE + _PAIRS + (_STRIDES + _STRIDE_PAIRS if general else [])
        if entry == "smc_basket_price_paths":
            rejected = rejected + _PATH_ONLY
        for case in rejected:
            for B in ((0, 1) if "B" not in case else (case["B"],)):
                out.append((entry, {**_BASE, **case, "B": B}))
        for bad_b in (-1, 1 << 31):
            out.append((entry, {**_BASE, "B": bad_b}))
        for case in _ACCEPTED + (_ACCEPTED_GENERAL if general else []):
            if all(k in names for k in case):
                out.append((entry, {**_BASE, **case, "B": 0}))
    train = [dict(contracts=None), dict(paths=None), dict(targets=None), dict(A=0), dict(A=9), dict(T=0), dict(N=0),
             dict(M=0), dict(N=6, M=1024), dict(N=8192, M=1), dict(M=31), dict(N=4096, M=1 << 17), dict(math=1),
             dict(math=REPLAY), dict(math=HW | REPLAY), dict(store=0), dict(store=7), dict(pitch=3), dict(pitch=2044),
             dict(pitch=2050), dict(chunk=0), dict(chunk=-1),
             # two at once
             dict(contracts=None, A=9), dict(A=9, T=0), dict(T=0, M=31), dict(M=31, math=1), dict(math=1, store=7),
             dict(store=7, pitch=3), dict(pitch=3, chunk=0)]
    for case in train:
        for B in (0, 1):
            out.append(("smc_basket_train_targets", {**_TRAIN_BASE, **case, "B": B}))
    for bad_b in (-1, 1 << 31):
        out.append(("smc_basket_train_targets", {**_TRAIN_BASE, "B": bad_b}))
    for case in (dict(), dict(sums=None), dict(norm=RAW), dict(norm=7), dict(math=HW, store=_lib.STORE_ALL, pitch=2052)):
        out.append(("smc_basket_train_targets", {**_TRAIN_BASE, **case, "B": 0}))
    return out


def positional(entry: str, kw: dict) -> list:
    return [kw[n] for n in (BATCHED[entry] if entry in BATCHED else _TRAIN)]


def _last_true(pred, lo: int, hi: int) -> int:
    """The largest x in [lo, hi) with pred(x), for a pred that is true up to some x and false beyond."""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def name_table(L) -> list[list]:
    """[entry, A, T, P, math, norm] of every recorded kernel-name query: per kernel and asset count P = 1, 2048, the
    last P that parks and the first that replays (found on the recorded library), every math and normalisation; the
    path kernel, which parks nothing, at its last fitting and first rejected number of dates instead; then the shapes
    and flags that are "unsupported"."""
    out: list[list] = []
    maths, norms = (0, HW, REPLAY, HW | REPLAY), (RAW, NORM)
    for entry in BATCHED:
        fn = getattr(L, entry + "_kernel")
        for A in range(1, 9):
            if entry == "smc_basket_price_paths":
                edge = _last_true(lambda T: fn(A, T, 693, 0, NORM) != b"unsupported", 1, 1 << 20)
                shapes = [(T, P) for T in (16, edge, edge + 1) for P in (1, 2048)]
            else:
                edge = _last_true(lambda P: fn(A, 16, P, 0, NORM).endswith(b"(lds)"), 1, 1 << 20)
                shapes = [(16, P) for P in (1, 2048, edge, edge + 1)]
            out += [[entry, A, T, P, math, norm] for T, P in shapes for math in maths for norm in norms]
        for norm in norms:
            out += [[entry, A, 16, 2048, 0, norm] for A in (0, 9, -1)]
            out += [[entry, 4, T, P, 0, norm] for T, P in ((0, 2048), (-1, 2048), (16, 0), (16, -4), (16, 1 << 40))]
            out += [[entry, 4, 16, 2048, math, norm] for math in (1, 0x2000, _lib.MATH_REF, _lib.TRAIN_DYNAMIC, -1)]
        out += [[entry, 4, 16, 2048, 0, norm] for norm in (7, -1, 2)]
    return out


def train_name_table() -> list[list]:
    """[A, T, N, M, with_sync, keep_sums] of smc_basket_train_targets_kernel's recorded queries (no HIP call)."""
    return [[A, T, N, M, sync, keep] for A in range(1, 9) for T, N, M in ((16, 256, 512), (16, 64, 32), (8, 256, 512))
            for sync in (0, 1) for keep in (0, 1)] + [[0, 16, 256, 512, 1, 1], [9, 16, 256, 512, 1, 0]]


def run_call(L, entry: str, args: list, buf: int) -> tuple[int, str | None]:
    """(status, last_error text or None for SMC_OK) of one recorded call; ``buf`` stands for every "buf"."""
    status = int(getattr(L, entry)(*[buf if a == BUF else a for a in args]))
    return status, (_lib.last_error() if status != _lib.SMC_OK else None)


def main() -> None:
    import ctypes

    L = _lib.lib()
    dummy = (ctypes.c_double * 128)()
    calls = []
    for entry, kw in call_table():
        args = positional(entry, kw)
        status, error = run_call(L, entry, args, ctypes.addressof(dummy))
        # nothing of the table may reach a launch
        assert kw["B"] == 0 or status in (_lib.SMC_ERR_INVALID_ARGUMENT, _lib.SMC_ERR_INVALID_SHAPE), (entry, kw)
        calls.append({"entry": entry, "args": args, "status": status, "error": error})
    assert all(v == 0.0 for v in dummy)
    names = [q + [getattr(L, q[0] + "_kernel")(*q[1:]).decode()] for q in name_table(L)]
    train_names = [q + [L.smc_basket_train_targets_kernel(*q).decode()] for q in train_name_table()]
    dst = os.path.join(HERE, "basket_host_errors.json")
    with open(dst, "w") as f:  # one record per line
        f.write("{\n")
        for key, rows in (("calls", calls), ("names", names), ("train_names", train_names)):
            f.write(f' "{key}": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]")
            f.write(",\n" if key != "train_names" else "\n")
        f.write("}\n")
    print(f"wrote {dst} from {_lib.LIB_PATH}: {len(calls)} calls, {len(names)} + {len(train_names)} kernel names")


if __name__ == "__main__":
    main()
