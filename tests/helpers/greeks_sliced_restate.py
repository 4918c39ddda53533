"""The portable float32 restatement of smc_gbm_greeks_sliced's [B][26] block: greeks_restate's table on the oracle's
kernel-mode terminal values, with the terminal sum taken slice by slice (price_sliced_restate.sliced_terminal:
oracle_kernel_paths at span = slice_paths, wg = 512, each slice in the 512-lane order, the slices added in order) and
the NORMALIZE constants (the scale F / f32(sumx / P), Lbar = sumxl / sumx) from that total.  Pure numpy and the oracle:
importable without a GPU.

The other sums (sum f64(x L) and the ten terms with their squares) are numpy's pairwise float64 sums, not the kernels'
order: hence the P 2^-52 bounds of the tests that compare them."""

from __future__ import annotations

import numpy as np

from tests.helpers import greeks_restate as restate
from tests.helpers import price_sliced_restate as psr

LOG_EULER = 0


def paths_f32(oracle, c: np.ndarray, T: int, P: int, slice_paths: int, seed: int,
              ordinal0: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(terminal values [B, P] f32, their portable logs L = log_pos(x / f32(X0)), the terminal sums in sliced order)."""
    term, tsum = psr.sliced_terminal(oracle, c, T, P, slice_paths, seed, ordinal0, LOG_EULER)
    L = restate.log_pos_f32(term / c[:, 0].astype(np.float32)[:, None])
    return term, L, tsum


def block_f32(oracle, c: np.ndarray, T: int, P: int, slice_paths: int, seed: int, ordinal0: int,
              norm: int) -> np.ndarray:
    """smc_gbm_greeks_sliced's block for the contracts c in portable f32 math."""
    term, L, tsum = paths_f32(oracle, c, T, P, slice_paths, seed, ordinal0)
    return restate.block(c, term, L, norm, tsum)
