"""The portable float32 restatement of smc_gbm_price_sliced's [B][8] block: gbm_restate.price_block on the oracle's
kernel-mode terminal values, with the terminal sum taken slice by slice (oracle_kernel_paths at span = slice_paths,
wg = 512: each slice in the 512-lane order, the slices added in order from 0.0) and the NORMALIZE scale
F / f32(tsum / P) from that total.  Pure numpy and the oracle: importable without a GPU.

The span is passed to the C entry point directly (oracle.kernel_paths derives it from a slice count, which needs
slices | P), so a ragged P works: the last slice ends at P.  The payoff sums are numpy's pairwise float64 sums, not
the kernels' order: hence the P 2^-52 bounds of the tests that compare columns 0..4."""

from __future__ import annotations

import numpy as np

from tests.helpers import gbm_restate as gr

f32 = np.float32


def sliced_terminal(oracle, c: np.ndarray, T: int, P: int, slice_paths: int, seed: int, ordinal0: int,
                    scheme: int) -> tuple[np.ndarray, np.ndarray]:
    """(terminal values [B, P] f32, terminal sum [B] f64 in the sliced order) of the contracts c."""
    oracle.build()
    assert slice_paths > 0 and slice_paths % 2048 == 0
    c = np.ascontiguousarray(c, dtype=np.float64)
    B = c.shape[0]
    terminal = np.empty((B, P), dtype=np.float32)
    rowsum = np.empty((B, T), dtype=np.float64)
    oracle.oracle.lib().oracle_kernel_paths(c.ctypes.data, B, T, P, seed, ordinal0, scheme, slice_paths, 512, None,
                                            terminal.ctypes.data, rowsum.ctypes.data)
    return terminal, rowsum[:, -1].copy()


def price_sliced_f32(oracle, c: np.ndarray, T: int, P: int, slice_paths: int, seed: int, ordinal0: int, scheme: int,
                     norm: int) -> dict[str, np.ndarray]:
    """smc_gbm_price_sliced's block for the contracts c in portable f32 math."""
    B = c.shape[0]
    term, tsum = sliced_terminal(oracle, c, T, P, slice_paths, seed, ordinal0, scheme)
    Tm = c[:, 2].astype(f32)
    F = c[:, 0].astype(f32) * gr.exp_any_f32(oracle, (c[:, 3] - c[:, 4]).astype(f32) * Tm)
    df = gr.exp_any_f32(oracle, (-c[:, 3]).astype(f32) * Tm)
    K = c[:, 1].astype(f32)
    s = F / (tsum / P).astype(f32) if norm else np.ones(B, dtype=f32)
    xs = term * s[:, None]
    assert xs.dtype == f32 and F.dtype == f32 and df.dtype == f32
    return gr.price_block(xs, K, F, df, tsum)
