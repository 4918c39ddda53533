"""The condition on the reference alone for the sliced Greeks call: the portable float32 restatement of
smc_gbm_greeks_sliced (tests/helpers/greeks_sliced_restate.py), at the W > 1 shapes and slice lengths of the GPU cases
(tests/test_gpu_greeks_sliced.py), lies within the a-priori bound of the independent float64 reference
(tests/helpers/greeks_reference.py) for the fourteen case rows, with the paths in doubt inside
gbm_reference.count_ok.  Every sum of that reference carries a P 2^-52 association term, so the sliced order needs no
new tolerance.  With one slice the restatement is greeks_restate.block_f32 exactly.  CPU only."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.helpers import gbm_reference as gref
from tests.helpers import greeks_reference as gk
from tests.helpers import greeks_restate as restate
from tests.helpers import greeks_sliced_restate as gsr
from tests.test_greeks_reference import ORD0, SEED, _oracle, case_rows

# (T, P, slice_paths): tests/test_gpu_greeks_sliced.py's W > 1 shapes
SLICED = [(16, 6837, 2048),   # W = 4: last slice of 693 paths
          (5, 10241, 4096),   # W = 3: two chunks per slice, last slice of one path
          (1, 4624, 2048),    # W = 3: the 16-path stream span across slice boundaries
          (2, 4624, 2048)]    # W = 3: the same at T = 2
ONE = [(16, 4096, 4096), (16, 693, 2048)]


@functools.lru_cache(maxsize=None)
def reference(T: int, P: int, normalize: bool, math: str = "portable") -> gk.GreeksRef:
    """The independent reference of the fourteen case rows at this shape (shared with the GPU tests)."""
    return gk.reference(_oracle(), case_rows(), T, P, SEED, ORD0, math=math, normalize=normalize)


@functools.lru_cache(maxsize=None)
def restated(T: int, P: int, span: int, normalize: bool) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        out = gsr.block_f32(_oracle(), case_rows(), T, P, span, SEED, ORD0, int(normalize))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("T,P,span", SLICED)
def test_sliced_restatement_within_the_bound(T, P, span) -> None:
    assert -(-P // span) > 1
    for normalize in (False, True):
        label = f"T {T} P {P} slice {span} {'NORMALIZE' if normalize else 'RAW'}"
        ref = reference(T, P, normalize)
        assert gref.count_ok(ref.doubt, P), (label, ref.doubt)  # a condition on the strikes, met by the reference alone
        got = restated(T, P, span, normalize)
        assert got.shape == (case_rows().shape[0], gk.COLS) and not np.isnan(got).any()
        used = gk.shares(got, ref)
        print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items())
              + f"; paths in doubt {int(ref.doubt.max())}")
        assert max(used.values()) < 1.0, (label, used)
        if not normalize:
            assert np.all(got[:, 25] == 0.0)


@pytest.mark.parametrize("T,P,span", ONE + [(5, 693, 1 << 20)])
def test_one_slice_is_the_unsliced_restatement(T, P, span) -> None:
    for normalize in (False, True):
        with np.errstate(divide="ignore", invalid="ignore"):
            want = restate.block_f32(case_rows(), T, P, SEED, ORD0, int(normalize))
        assert restated(T, P, span, normalize).tobytes() == want.tobytes(), (T, P, span, normalize)


def test_sliced_restatement_differs_from_the_unsliced_one_in_its_last_bits_only() -> None:
    """More than one slice: the terminal values are the same, the terminal sum is associated by slice, so the two
    restatements agree to the sum-order bound P 2^-52 of the total, not necessarily bit for bit."""
    T, P, span = SLICED[1]
    oracle = _oracle()
    rows = case_rows()
    term, _, tsum = gsr.paths_f32(oracle, rows, T, P, span, SEED, ORD0)
    _, whole, rs = oracle.kernel_paths(rows, T, P, SEED, ORD0, 0)
    assert term.tobytes() == whole.tobytes()
    np.testing.assert_allclose(tsum, rs[:, -1], rtol=P * 2.0 ** -52, atol=0)
    assert restated(T, P, span, True)[:, 24].tobytes() == tsum.tobytes()
