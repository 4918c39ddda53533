"""greeks_kernel (smc_gbm_greeks) against the independent float64 reference of tests/helpers/greeks_reference.py, in
portable and in SMC_MATH_HW math: all 26 columns within the a-priori bound the helper derives from the reference's own
values (computed before the kernel's output is looked at), into a NaN-poisoned block.  SMC_MATH_HW has no CPU
restatement (hw_log, the HW path kernels): this file is what holds its raw, lds and replay instantiations, at ragged
P, P < 512, T <= 2 and odd T.  The float64 instantiations are held to the same reference on the float64 engine's
uniforms at the project's float64 tolerance.

Each case asserts the name of the kernel it means to reach.  The contracts are those of the CPU sweep
(tests/test_greeks_reference.case_rows), whose strikes keep the paths in doubt within gbm_reference.count_ok."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import oracle as _oracle
from spectralmc_amd import _lib
from tests.helpers import ATOL_FLOAT64, RTOL_FLOAT64, poisoned
from tests.helpers import gbm_reference as gref
from tests.helpers import greeks_reference as gk
from tests.helpers import instantiations as inst
from tests.test_greeks_reference import ORD0, SEED, case_rows, degenerate_rows

pytestmark = pytest.mark.gpu

DEV = "cuda"
MATHS = {"portable": 0, "hw": _lib.MATH_HW}
RAW, NORM = _lib.NORM_RAW, _lib.NORM_NORMALIZE
F32_PARK = 36784  # the largest P whose f32 terminal row is parked in LDS (tests/test_greeks_host.py finds it)
F64_PARK = 14036


def _rows(B: int) -> np.ndarray:
    """The first B case rows, taken round again where B is larger than the set."""
    rows = case_rows()
    return rows[np.arange(B) % rows.shape[0]]


def _greeks(rows: np.ndarray, T: int, P: int, flags: int, norm: int, dtype: int) -> np.ndarray:
    cd = torch.tensor(rows, dtype=torch.float64, device=DEV)
    out = poisoned((rows.shape[0], _lib.GREEKS_COLS), torch.float64, DEV)
    _lib.check(_lib.lib().smc_gbm_greeks(_lib.ptr(cd), rows.shape[0], T, P, SEED, None, ORD0, flags, norm, dtype,
                                         _lib.ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _name(T: int, P: int, flags: int, norm: int, dtype: int) -> str:
    return _lib.lib().smc_gbm_greeks_kernel(T, P, flags, norm, dtype).decode()


def _hold(rows: np.ndarray, T: int, P: int, mode: str, flags: int, norm: int) -> None:
    """One shape in both maths: the reference and its bound first, then the kernel."""
    _oracle.build()
    for math, hw in MATHS.items():
        ref = gk.reference(_oracle, rows, T, P, SEED, ORD0, math=math, normalize=norm == NORM)
        assert gref.count_ok(ref.doubt, P), ref.doubt  # the condition on the strikes, on the reference alone
        assert _name(T, P, flags | hw, norm, _lib.DTYPE_F32) == f"greeks_kernel({mode})"
        got = _greeks(rows, T, P, flags | hw, norm, _lib.DTYPE_F32)
        label = f"greeks_kernel({mode}) B {rows.shape[0]} T {T} P {P} {math}"
        assert got.shape == (rows.shape[0], gk.COLS) and not np.isnan(got).any(), label
        used = gk.shares(got, ref)
        print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
              + f"; paths in doubt {int(ref.doubt.max())}")
        assert max(used.values()) < 1.0, (label, used)
        if norm == RAW:
            assert np.all(got[:, 25] == 0.0), label


# (mode, B, T, P, flags): one pass at a whole chunk count and at P < 512 with an even T; parked rows at two whole chunks,
# an odd T with a ragged P, the stream span at T = 1 and T = 2 (the latter at P < 512), an odd T beyond one row block;
# replay forced at a ragged P; replay chosen by the shape one path beyond the park bound (a ragged P again); more
# contracts than CUs; a single path
CASES = [
    ("raw", 12, 3, 2048, 0),
    ("raw", 12, 16, 21, 0),
    ("lds", 12, 16, 4096, 0),
    ("lds", 12, 5, 693, 0),
    ("lds", 12, 1, 528, 0),
    ("lds", 12, 2, 21, 0),
    ("lds", 12, 17, 1024, 0),
    ("replay", 12, 16, 693, _lib.PRICE_REPLAY),
    ("replay", 3, 3, F32_PARK + 1, 0),
    ("lds", 300, 3, 528, 0),
    ("raw", 12, 4, 1, 0),
    ("lds", 12, 4, 1, 0),
    ("replay", 12, 4, 1, _lib.PRICE_REPLAY),
]


@pytest.mark.parametrize("mode,B,T,P,flags", CASES)
def test_greeks_kernel_within_the_bound(mode, B, T, P, flags) -> None:
    if P == F32_PARK + 1:
        assert _name(T, F32_PARK, 0, NORM, _lib.DTYPE_F32) == "greeks_kernel(lds)"
    # the launches the ledger counts for the row are the ones _hold makes: both maths in the mode the row states
    runs = inst.pricing_runs_of("greeks f32", (mode, B, T, P, flags))
    assert [(r.math, r.name, r.force_replay, r.normalize) for r in runs] == \
        [(m, f"greeks_kernel({mode})", bool(flags), mode != "raw") for m in MATHS]
    _hold(_rows(B), T, P, mode, flags, RAW if mode == "raw" else NORM)


@pytest.mark.parametrize("mode,flags,norm", [("raw", 0, RAW), ("lds", 0, NORM), ("replay", _lib.PRICE_REPLAY, NORM)])
def test_greeks_kernel_degenerate_rows_within_the_bound(mode, flags, norm) -> None:
    """v = 0 (vega, gamma and their errors exactly 0), the T v^2 corner (q far outside [2^-8, 2^8)), the flat row,
    T = 0 and v = 0.01 (the worst RAW cancellation in hv)."""
    rows = degenerate_rows()
    _hold(rows, 8, 256, mode, flags, norm)
    got = _greeks(rows, 8, 256, flags, norm, _lib.DTYPE_F32)
    assert np.all(got[[0, 2]][:, [2, 3, 8, 9, 12, 13, 18, 19]] == 0.0)  # v == 0
    assert np.all(got[3, [8, 9, 18, 19]] == 0.0)                        # T == 0


# the last shape lies just under the f64 park bound
F64_CASES = [(16, 4096), (5, 693), (2, F64_PARK - 36)]


@pytest.mark.parametrize("T,P", F64_CASES)
def test_greeks_kernel_f64_against_the_reference(T, P) -> None:
    _oracle.build()
    rows = _rows(12)
    assert _name(T, F64_PARK, 0, NORM, _lib.DTYPE_F64) == "greeks_kernel(lds)"
    assert _name(T, F64_PARK + 1, 0, NORM, _lib.DTYPE_F64) == "greeks_kernel(replay)"
    runs = inst.pricing_runs_of("greeks f64", (T, P))  # every launch the ledger counts for the row
    assert [r.name for r in runs] == ["greeks_kernel(raw)", "greeks_kernel(lds)", "greeks_kernel(replay)"]
    for run in runs:
        mode, flags, norm = run.name[14:-1], (_lib.PRICE_REPLAY if run.force_replay else 0), (NORM if run.normalize else RAW)
        ref = _f64_reference(T, P, norm == NORM)
        assert _name(T, P, flags, norm, _lib.DTYPE_F64) == f"greeks_kernel({mode})"
        got = _greeks(rows, T, P, flags, norm, _lib.DTYPE_F64)
        assert not np.isnan(got).any(), mode
        share = np.abs(got - ref.cols) / gk.tol64(ref, RTOL_FLOAT64, ATOL_FLOAT64)
        print(f"greeks_kernel({mode}) f64 T {T} P {P}: largest share of the f64 tolerance {share.max():.3e} "
              f"(column {int(share.max(axis=0).argmax())})")
        assert np.all(share <= 1.0), (mode, np.argwhere(share > 1.0).tolist())


@functools.lru_cache(maxsize=2)
def _f64_reference(T: int, P: int, normalize: bool) -> gk.GreeksRef:
    return gk.reference(_oracle, _rows(12), T, P, SEED, ORD0, normalize=normalize, f64=True)
