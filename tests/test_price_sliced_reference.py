"""The condition on the reference alone for the sliced pricing call: the portable float32 restatement of
smc_gbm_price_sliced (tests/helpers/price_sliced_restate.py), at the shapes and slice lengths of the GPU cases
(tests/test_gpu_price_sliced.py), lies within the a-priori price bound of the independent float64 reference
(tests/helpers/gbm_reference.py) for the twelve case rows.  That bound holds for any association of the f64 sums
(row_sums and mean_and_stderr carry a P 2^-52 term; the f32 4-path partial is unchanged), so the sliced order needs
no new tolerance.  With one slice the restatement is gbm_restate.price_f32 exactly.  CPU only."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests.helpers import gbm_reference as gref
from tests.helpers import gbm_restate as gr
from tests.helpers import price_sliced_restate as psr
from tests.test_gbm_reference import ORD0, SEED, _oracle, case_rows

LOG, SIMPLE = gref.LOG_EULER, gref.SIMPLE_EULER
# (T, P, slice_paths, scheme): tests/test_gpu_price_sliced.py's shapes
SHAPES = [(16, 6837, 2048, LOG), (5, 10241, 4096, LOG), (1, 4624, 2048, LOG), (2, 4624, 2048, LOG),
          (16, 4096, 4096, LOG), (16, 693, 2048, LOG), (5, 6837, 2048, SIMPLE)]


@functools.lru_cache(maxsize=None)
def reference(T: int, P: int, scheme: int, normalize: bool, math: str = "portable") -> gref.GbmRef:
    """The independent reference of the twelve case rows at this shape (shared with the GPU tests)."""
    rows, _ = case_rows(scheme, normalize)
    eps = {"portable": gref.F32_PORTABLE, "hw": gref.F32_HW}[math]
    return gref.reference(_oracle(), rows, T, P, SEED, ORD0, scheme=scheme, eps=eps, normalize=normalize)


@functools.lru_cache(maxsize=None)
def restated(T: int, P: int, span: int, scheme: int, normalize: bool) -> dict[str, np.ndarray]:
    rows, _ = case_rows(scheme, normalize)
    return psr.price_sliced_f32(_oracle(), rows, T, P, span, SEED, ORD0, scheme, int(normalize))


@pytest.mark.parametrize("T,P,span,scheme", SHAPES)
def test_sliced_restatement_within_the_bound(T, P, span, scheme) -> None:
    for normalize in (False, True):
        ref = reference(T, P, scheme, normalize)
        got = restated(T, P, span, scheme, normalize)["cols"]
        assert got.shape == (12, 8) and not np.isnan(got).any()
        used = {"means": gref.share_used(got[:, :3], ref.price[:, :3], ref.price_bound[:, :3]),
                "stderr": gref.share_used(got[:, 3:5], ref.price[:, 3:5], ref.price_bound[:, 3:5]),
                "intrinsic": gref.share_used(got[:, 5:7], ref.price[:, 5:7], ref.price_bound[:, 5:7]),
                "terminal sum": gref.share_used(got[:, 7], ref.price[:, 7], ref.price_bound[:, 7])}
        label = (f"T {T} P {P} slice {span} {'log' if scheme == LOG else 'simple'} Euler "
                 f"{'NORMALIZE' if normalize else 'RAW'}")
        print(f"{label}: share of the bound used " + ", ".join(f"{k} {v:.3f}" for k, v in used.items()))
        assert max(used.values()) < 1.0, (label, used)


@pytest.mark.parametrize("T,P,span,scheme", [s for s in SHAPES if s[2] >= s[1]] + [(5, 693, 1 << 20, SIMPLE)])
def test_one_slice_is_the_unsliced_restatement(T, P, span, scheme) -> None:
    rows, _ = case_rows(scheme, True)
    for normalize in (False, True):
        want = gr.price_f32(_oracle(), rows, T, P, SEED, ORD0, scheme, int(normalize))["cols"]
        got = restated(T, P, span, scheme, normalize)["cols"]
        assert got.tobytes() == want.tobytes(), (T, P, span, normalize)


def test_sliced_terminal_sum_is_the_slices_in_order() -> None:
    """What the helper's span means: per slice the 512-lane order over the slice's own chunks, the slices added in
    order; so a sliced total differs from the unsliced one in its last bits at most, and the terminal values not at
    all."""
    rows, _ = case_rows(LOG, True)
    oracle = _oracle()
    T, P, span = 5, 10241, 4096
    term, tsum = psr.sliced_terminal(oracle, rows, T, P, span, SEED, ORD0, LOG)
    _, whole, rs = oracle.kernel_paths(rows, T, P, SEED, ORD0, LOG)
    assert term.tobytes() == whole.tobytes()
    parts = []
    for p0 in range(0, P, span):  # a slice alone, as its own "contract" of the lanes' partial sums
        x = np.zeros((rows.shape[0], span), dtype=np.float32)
        x[:, :min(span, P - p0)] = whole[:, p0:p0 + span]
        quad = x.reshape(-1, span // 2048, 512, 4)
        part = ((quad[..., 0] + quad[..., 1]) + quad[..., 2]) + quad[..., 3]  # f32, paths ascending
        lane = np.zeros((rows.shape[0], 512))
        for ch in range(span // 2048):
            lane = lane + part[:, ch].astype(np.float64)
        v = lane.reshape(-1, 8, 64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[:, :, np.arange(64) ^ off]
        tot = np.zeros(rows.shape[0])
        for w in range(8):
            tot = tot + v[:, w, 0]
        parts.append(tot)
    total = parts[0]
    for part in parts[1:]:
        total = total + part
    assert total.tobytes() == tsum.tobytes()
    np.testing.assert_allclose(tsum, rs[:, -1], rtol=P * 2.0 ** -52, atol=0)
