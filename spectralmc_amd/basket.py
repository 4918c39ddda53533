"""Correlated multi-asset GBM (basket) engine — BASELINE.json configs[4] extension.

The reference prices one asset per contract (``src/spectralmc/gbm.py``).  This module adds
the builder-defined multi-asset case the benchmark names ("multi-asset correlated GBM, 4
assets, Cholesky in LDS"): each asset follows the reference log-Euler dynamics
(gbm.py:224-257) and forward normalisation (gbm.py:428-440), the assets' Brownian drivers
are equicorrelated with a per-contract rho, the payoff is an equal-weight basket put, and
the training target is mean_m FFT_N(put.reshape(M, N)) as ``_simulate_fft``
(gbm_trainer.py:806-817).

Contract row (Sobol dimensions, in order): K, T, r, rho, X0_0..X0_{A-1}, d_0..d_{A-1},
v_0..v_{A-1}.  All device work is one launch of ``smc_basket_train_targets`` (csrc/basket.hip)
per chunk of contracts, after the Sobol draw; no host synchronisation.

``BasketEngine`` has the interface of ``engine.TrainingEngine`` (``buffers``,
``enqueue_step``, ``set_position``, ``global_batch``), so a ``GbmCVNNPricer`` whose CVNN has
3A+4 inputs trains on baskets through ``use_basket_engine``.  Snapshots of such a pricer
record the network, optimizer and Sobol/normal positions as usual but not the basket
configuration: call ``use_basket_engine`` again on the restored pricer.  ``predict_price``
stays single-asset; the Monte-Carlo price of a basket (and of the best-of / worst-of payoffs on the
same paths) comes from ``basket_price`` / ``BasketEngine.price``: one launch of ``smc_basket_price`` for
B contracts, no terminal buffer in memory; with ``weights=`` and / or ``correlation=`` the basket has the caller's
weights and full correlation matrix (``smc_basket_price_general``).  ``basket_greeks`` / ``BasketEngine.greeks``
give the basket put's and call's per-asset deltas and vegas, rho, theta and correlation sensitivity the same way
(``smc_basket_greeks``; with ``weights=`` and / or ``correlation=`` those of the weighted, general-correlation basket, the
correlation sensitivity per pair: ``smc_basket_greeks_general``).  ``basket_price_paths`` / ``BasketEngine.price_paths``
price the path-dependent payoffs of that basket over the monitoring dates (Asian, knock-out, lookback, worst-of
knock-out: ``smc_basket_price_paths``); ``basket_greeks_paths`` / ``BasketEngine.greeks_paths`` give the per-asset
deltas and vegas, rho and theta of the Asian and lookback ones (``smc_basket_greeks_paths``).
"""

from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from . import engine as _engine
from .engine import StepBuffers, check_sync_status
from .sobol_sampler import SobolEngine, draw_device

MAX_ASSETS = 8


def basket_fields(n_assets: int) -> tuple[str, ...]:
    return ("K", "T", "r", "rho") + tuple(f"X0_{i}" for i in range(n_assets)) + tuple(
        f"d_{i}" for i in range(n_assets)) + tuple(f"v_{i}" for i in range(n_assets))


def default_basket_bounds(n_assets: int, *, x0=(0.001, 10_000.0), k=(0.001, 20_000.0), t=(0.0, 10.0),
                          r=(-0.20, 0.20), d=(-0.20, 0.20), v=(0.0, 2.0),
                          rho=None) -> dict[str, tuple[float, float]]:
    """Per-field (lower, upper): the single-asset defaults of tests/helpers/factories.py:108-161
    per asset, plus the correlation range (default [max(-0.2, -0.9/(A-1)), 0.9]: the
    equicorrelation matrix is positive definite for rho > -1/(A-1))."""
    if rho is None:
        rho = (max(-0.20, -0.9 / (n_assets - 1)) if n_assets > 1 else -0.20, 0.90)
    out = {"K": k, "T": t, "r": r, "rho": rho}
    for i in range(n_assets):
        out[f"X0_{i}"] = x0
    for i in range(n_assets):
        out[f"d_{i}"] = d
    for i in range(n_assets):
        out[f"v_{i}"] = v
    return out


@dataclass(frozen=True)
class BasketConfig:
    n_assets: int = 4
    timesteps: int = 16
    network_size: int = 256
    batches_per_mc_run: int = 512
    mc_seed: int = 7
    normalize: bool = True
    math: str = "hw"  # "hw" (hardware transcendentals) or "portable" (bit-identical to the oracle)
    bounds: dict[str, tuple[float, float]] | None = field(default=None)

    def __post_init__(self) -> None:
        if not 1 <= self.n_assets <= MAX_ASSETS:
            raise ValueError(f"n_assets must be in 1..{MAX_ASSETS}, got {self.n_assets}")
        if self.timesteps <= 0 or self.network_size <= 0 or self.batches_per_mc_run <= 0:
            raise ValueError("timesteps, network_size and batches_per_mc_run must be positive")
        if self.network_size % 4 or self.network_size > 4096:
            raise ValueError("network_size must be a multiple of 4 and <= 4096")
        if self.total_paths % 2048:
            raise ValueError("network_size * batches_per_mc_run must be a multiple of 2048")
        if self.math not in ("hw", "portable"):
            raise ValueError(f"math must be 'hw' or 'portable', got {self.math!r}")
        lo_rho = self.resolved_bounds()["rho"][0]
        if self.n_assets > 1 and lo_rho <= -1.0 / (self.n_assets - 1):
            raise ValueError(f"rho lower bound {lo_rho} makes the correlation matrix indefinite")

    @property
    def total_paths(self) -> int:
        return self.network_size * self.batches_per_mc_run

    @property
    def dim(self) -> int:
        return 3 * self.n_assets + 4

    def resolved_bounds(self) -> dict[str, tuple[float, float]]:
        b = default_basket_bounds(self.n_assets)
        if self.bounds:
            unknown = set(self.bounds) - set(b)
            if unknown:
                raise ValueError(f"unknown basket fields {sorted(unknown)}")
            b.update(self.bounds)
        return b

    def arrays(self) -> tuple[np.ndarray, np.ndarray]:
        b = self.resolved_bounds()
        names = basket_fields(self.n_assets)
        return (np.array([b[n][0] for n in names], dtype=np.float64),
                np.array([b[n][1] for n in names], dtype=np.float64))


def sync_bytes(cfg: BasketConfig, chunk_contracts: int) -> int:
    """Bytes of the sync area the resident basket kernel needs for this shape and launch size (0: it
    does not take the shape)."""
    n = int(_lib.lib().smc_basket_sync_bytes(cfg.n_assets, cfg.timesteps, cfg.network_size, cfg.batches_per_mc_run,
                                             chunk_contracts))
    if n < 0:
        raise RuntimeError("smc_basket_sync_bytes: bad shape or device query failed")
    return n


def basket_targets(contracts: torch.Tensor, cfg: BasketConfig, *, ordinal0: int = 0, paths: torch.Tensor | None = None,
                   terminal_sum: torch.Tensor | None = None, targets: torch.Tensor | None = None,
                   pitch: int = 0, resident: bool = True) -> torch.Tensor:
    """One call of the basket engine on explicit device contracts [B, 3A+4] f64.
    ``paths``: [B, A, T, pitch] f32 to keep every row, else only terminal rows are kept (scratch).
    ``resident``: pass a sync area, so shapes basket_resident_kernel takes run it (reduction orders:
    oracle.basket_order(...))."""
    _lib.require_device()
    B = contracts.shape[0]
    if contracts.dtype != torch.float64 or contracts.shape[1] != cfg.dim or not contracts.is_contiguous():
        raise ValueError(f"contracts must be a contiguous (B, {cfg.dim}) float64 tensor")
    P = cfg.total_paths
    pitch = pitch or P
    store = _lib.STORE_ALL if paths is not None else _lib.STORE_TERMINAL
    if paths is None:
        paths = torch.empty((B, cfg.n_assets, pitch), dtype=torch.float32, device=contracts.device)
    elif paths.dtype != torch.float32 or paths.numel() < B * cfg.n_assets * cfg.timesteps * pitch:
        raise ValueError("paths must be float32 with room for [B, A, T, pitch]")
    if targets is None:
        targets = torch.empty((B, cfg.network_size), dtype=torch.complex64, device=contracts.device)
    nsync = sync_bytes(cfg, max(B, 1)) if resident else 0
    sync = torch.zeros(nsync, dtype=torch.uint8, device=contracts.device) if nsync else None
    _lib.check(_lib.lib().smc_basket_train_targets(
        _lib.ptr(contracts), B, cfg.n_assets, cfg.timesteps, cfg.network_size, cfg.batches_per_mc_run, cfg.mc_seed,
        None, ordinal0, _lib.MATH_HW if cfg.math == "hw" else 0, 1 if cfg.normalize else 0, store, _lib.ptr(paths),
        pitch, max(B, 1), _lib.ptr(terminal_sum), _lib.ptr(targets), _lib.ptr(sync), nsync, _lib.stream_handle()))
    return targets


PRICE_FIELDS = ("basket_put", "basket_call", "best_of_put", "best_of_call", "worst_of_put", "worst_of_call",
                "basket_put_stderr", "basket_call_stderr", "best_of_put_stderr", "best_of_call_stderr",
                "worst_of_put_stderr", "worst_of_call_stderr", "mean_basket", "mean_best", "mean_worst",
                "put_exercise_share", "basket_put_intrinsic", "basket_call_intrinsic")


@dataclass(frozen=True)
class BasketPrices:
    """``smc_basket_price``'s block for B contracts: one [B] f64 device tensor per column (views of
    ``block`` [B, 18], in ``PRICE_FIELDS`` order) and the raw terminal sums ``terminal_sum`` [B, A]."""
    basket_put: torch.Tensor
    basket_call: torch.Tensor
    best_of_put: torch.Tensor
    best_of_call: torch.Tensor
    worst_of_put: torch.Tensor
    worst_of_call: torch.Tensor
    basket_put_stderr: torch.Tensor
    basket_call_stderr: torch.Tensor
    best_of_put_stderr: torch.Tensor
    best_of_call_stderr: torch.Tensor
    worst_of_put_stderr: torch.Tensor
    worst_of_call_stderr: torch.Tensor
    mean_basket: torch.Tensor
    mean_best: torch.Tensor
    mean_worst: torch.Tensor
    put_exercise_share: torch.Tensor
    basket_put_intrinsic: torch.Tensor
    basket_call_intrinsic: torch.Tensor
    terminal_sum: torch.Tensor
    block: torch.Tensor


def pack_correlation(C: torch.Tensor) -> torch.Tensor:
    """The strict lower triangle of correlation matrices ``[A, A]`` or ``[B, A, A]``, row by row ((1,0), (2,0),
    (2,1), (3,0), ...): the ``[A (A - 1) / 2]`` / ``[B, A (A - 1) / 2]`` rows ``smc_basket_price_general`` reads.  On
    the matrix's device, no host synchronisation; the upper triangle and the diagonal are not looked at."""
    if C.dim() not in (2, 3) or C.shape[-1] != C.shape[-2]:
        raise ValueError(f"a correlation matrix must be [A, A] or [B, A, A], got {tuple(C.shape)}")
    A = C.shape[-1]
    return C.reshape(C.shape[:-2] + (A * A,)).index_select(-1, _tril_flat(A, C.device)).contiguous()


@functools.lru_cache(maxsize=None)
def _tril_flat(A: int, device: torch.device) -> torch.Tensor:
    """Flat indices i A + k of the strict lower triangle in row-major order, on ``device`` (made once per asset
    count and device, so a later ``pack_correlation`` is device work only and can be captured into a graph)."""
    rows, cols = np.tril_indices(A, -1)
    return torch.from_numpy(rows * A + cols).to(device)


def unpack_correlation(tri: torch.Tensor, n_assets: int) -> torch.Tensor:
    """Packed rows ``[.., A (A - 1) / 2]`` (``pack_correlation``'s order) as symmetric matrices ``[.., A, A]`` with a zero
    diagonal: entry (j, k) and entry (k, j) both hold the row's value for the pair, so ``pack_correlation`` of the
    result is ``tri`` again.  The layout of ``BasketGeneralGreeks.correlation_put`` / ``correlation_call``, whose
    matrix form is the sensitivity to each pair.  On the rows' device, no host synchronisation."""
    A = n_assets
    if not 1 <= A <= MAX_ASSETS:
        raise ValueError(f"n_assets must be in 1..{MAX_ASSETS}, got {n_assets}")
    if tri.dim() < 1 or tri.shape[-1] != A * (A - 1) // 2:
        raise ValueError(f"packed rows must end in A (A - 1) / 2 = {A * (A - 1) // 2} entries, got {tuple(tri.shape)}")
    flat = torch.zeros(tri.shape[:-1] + (A * A,), dtype=tri.dtype, device=tri.device)
    if A > 1:
        flat.index_copy_(-1, _tril_flat(A, tri.device), tri)
    full = flat.reshape(tri.shape[:-1] + (A, A))
    return full + full.transpose(-1, -2)


def _general_weights(weights: torch.Tensor, B: int, A: int) -> tuple[torch.Tensor, int]:
    """(tensor, stride) of ``basket_price``'s ``weights``: [A] shared (stride 0) or [B, A] (stride A)."""
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64 or not weights.is_contiguous() or \
            tuple(weights.shape) not in ((A,), (B, A)):
        raise ValueError(f"weights must be a contiguous float64 tensor of shape ({A},) or ({B}, {A})")
    return weights, (0 if weights.dim() == 1 else A)


def _general_correlation(corr: torch.Tensor, B: int, A: int) -> tuple[torch.Tensor, int, bool]:
    """(tensor, stride, packed) of ``basket_price``'s ``correlation``: full matrices [A, A] / [B, A, A] or packed
    rows [A (A - 1) / 2] / [B, A (A - 1) / 2].  Shapes that read both ways (A = 3: [3, 3] is a matrix and, at
    B = 3, three packed rows) are taken as matrices."""
    n = A * (A - 1) // 2
    full = ((A, A), (B, A, A))
    if not isinstance(corr, torch.Tensor) or corr.dtype != torch.float64 or not corr.is_contiguous() or \
            tuple(corr.shape) not in full + ((n,), (B, n)):
        raise ValueError(f"correlation must be a contiguous float64 tensor of shape ({A}, {A}), ({B}, {A}, {A}), "
                         f"({n},) or ({B}, {n})")
    if tuple(corr.shape) in full:
        return corr, (0 if corr.dim() == 2 else n), False
    return corr, (0 if corr.dim() == 1 else n), True


def validate_basket_inputs(weights: torch.Tensor | None, correlation: torch.Tensor | None, n_assets: int) -> None:
    """``basket_price(validate=True)``'s checks (they read the values: a host synchronisation for device tensors):
    ValueError for a non-finite weight, and for a correlation matrix that is asymmetric, has a diagonal other than
    1 or is not positive definite (``torch.linalg.cholesky_ex``'s info).  Packed rows are unpacked into the
    symmetric unit-diagonal matrix they stand for, so only the last check can fail for them."""
    A = n_assets
    if weights is not None and not bool(torch.isfinite(weights).all()):
        raise ValueError("weights must be finite")
    if correlation is None:
        return
    C = correlation
    if not (C.dim() in (2, 3) and C.shape[-1] == A and C.shape[-2] == A):  # packed rows
        rows, cols = np.tril_indices(A, -1)
        full = torch.zeros(C.shape[:-1] + (A, A), dtype=C.dtype, device=C.device)
        full[..., torch.from_numpy(rows).to(C.device), torch.from_numpy(cols).to(C.device)] = C
        C = full + full.transpose(-1, -2) + torch.eye(A, dtype=C.dtype, device=C.device)
    if not bool(torch.isfinite(C).all()):
        raise ValueError("correlation must be finite")
    if not bool((C == C.transpose(-1, -2)).all()):
        raise ValueError("correlation must be symmetric")
    if not bool((torch.diagonal(C, dim1=-2, dim2=-1) == 1.0).all()):
        raise ValueError("correlation must have a unit diagonal")
    _, info = torch.linalg.cholesky_ex(C)
    if bool((info != 0).any()):
        raise ValueError("correlation must be positive definite")


@dataclass(frozen=True)
class _BatchedCall:
    """What ``basket_price``, ``basket_greeks`` and ``basket_price_paths`` hand to the library after the shared
    checks: the shape, the prepared ``weights`` and packed correlation rows ``tri`` with their strides (None and 0
    where not given) and the ``math`` / ``norm`` flags."""
    B: int
    A: int
    P: int
    general: bool
    weights: torch.Tensor | None
    w_stride: int
    tri: torch.Tensor | None
    c_stride: int
    math: int
    norm: int


def _batched_call(contracts: torch.Tensor, cfg: BasketConfig, n_paths: int | None, weights: torch.Tensor | None,
                  correlation: torch.Tensor | None, validate: bool, *, replay: bool = False,
                  barriers: torch.Tensor | None = None) -> _BatchedCall:
    """The checks the batched calls share, in their order: the tensors' shapes before the device is asked for, their
    placement after it, then ``validate``'s look at the values."""
    if contracts.dim() != 2 or contracts.dtype != torch.float64 or contracts.shape[1] != cfg.dim or \
            not contracts.is_contiguous():
        raise ValueError(f"contracts must be a contiguous (B, {cfg.dim}) float64 tensor")
    P = cfg.total_paths if n_paths is None else int(n_paths)
    if P <= 0:
        raise ValueError(f"n_paths must be positive, got {n_paths}")
    B, A = contracts.shape[0], cfg.n_assets
    if barriers is not None and (not isinstance(barriers, torch.Tensor) or barriers.dtype != torch.float64 or
                                 not barriers.is_contiguous() or tuple(barriers.shape) != (B, 3)):
        raise ValueError(f"barriers must be a contiguous float64 tensor of shape ({B}, 3)")
    general = weights is not None or correlation is not None
    w_stride = c_stride = 0
    packed = True
    if weights is not None:
        weights, w_stride = _general_weights(weights, B, A)
    if correlation is not None:
        correlation, c_stride, packed = _general_correlation(correlation, B, A)
    given = (("barriers", barriers), ("weights", weights), ("correlation", correlation))
    for name, t in given:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor")
    _lib.require_device()
    if not contracts.is_cuda:
        raise ValueError("contracts must be a device tensor")
    for name, t in given:
        if t is not None and t.device != contracts.device:
            raise ValueError(f"{name} must be on the contracts' device")
    if validate:
        validate_basket_inputs(weights, correlation, A)
        validate_basket_barriers(barriers)
    tri = None
    if B > 0 and correlation is not None:
        tri = correlation if packed else pack_correlation(correlation)
        if tri.numel() == 0:  # A = 1: no entry to read
            tri = None
    return _BatchedCall(B=B, A=A, P=P, general=general, weights=weights, w_stride=w_stride, tri=tri, c_stride=c_stride,
                        math=(_lib.MATH_HW if cfg.math == "hw" else 0) | (_lib.PRICE_REPLAY if replay else 0),
                        norm=_lib.NORM_NORMALIZE if cfg.normalize else _lib.NORM_RAW)


def basket_price(contracts: torch.Tensor, cfg: BasketConfig, *, ordinal0: int = 0, n_paths: int | None = None,
                 replay: bool = False, weights: torch.Tensor | None = None, correlation: torch.Tensor | None = None,
                 validate: bool = False) -> BasketPrices:
    """Monte-Carlo prices of the basket, best-of and worst-of puts and calls of device contracts [B, 3A+4]
    f64: one launch of ``smc_basket_price`` on the current stream, no host synchronisation.  ``cfg`` gives
    n_assets, timesteps, mc_seed, normalize and math; ``n_paths`` (default ``cfg.total_paths``) may be any
    positive count.  ``replay``: never park the terminal values in LDS (the same bits, for timing).

    ``weights`` / ``correlation`` (either one given: one launch of ``smc_basket_price_general`` instead):
    contiguous float64 device tensors.  ``weights`` [A] (shared by every contract) or [B, A]; any finite value,
    negatives included (spreads), not normalised; None means 1 / A.  ``correlation`` [A, A] or [B, A, A] (packed
    here with ``pack_correlation``), or already packed [A (A - 1) / 2] / [B, A (A - 1) / 2]; None means the rows'
    equicorrelation ``rho``, otherwise that column is ignored.  The values are not checked on the device
    (an indefinite matrix gives non-finite or meaningless rows); ``validate=True`` checks them here first
    (``validate_basket_inputs``) and is the only path that synchronises."""
    c = _batched_call(contracts, cfg, n_paths, weights, correlation, validate, replay=replay)
    B, A = c.B, c.A
    block = torch.empty((B, _lib.BASKET_PRICE_COLS), dtype=torch.float64, device=contracts.device)
    tsum = torch.empty((B, A), dtype=torch.float64, device=contracts.device)
    if B > 0 and c.general:
        _lib.check(_lib.lib().smc_basket_price_general(
            _lib.ptr(contracts), _lib.ptr(c.weights), c.w_stride, _lib.ptr(c.tri), c.c_stride, B, A, cfg.timesteps,
            c.P, cfg.mc_seed, None, ordinal0, c.math, c.norm, _lib.ptr(block), _lib.ptr(tsum), _lib.stream_handle()))
    elif B > 0:
        _lib.check(_lib.lib().smc_basket_price(
            _lib.ptr(contracts), B, A, cfg.timesteps, c.P, cfg.mc_seed, None, ordinal0, c.math, c.norm,
            _lib.ptr(block), _lib.ptr(tsum), _lib.stream_handle()))
    return BasketPrices(**{name: block[:, col] for col, name in enumerate(PRICE_FIELDS)}, terminal_sum=tsum,
                        block=block)


BASKET_PATH_FIELDS = ("asian_put", "asian_call", "knock_out_put", "knock_out_call", "lookback_put", "lookback_call",
                      "worst_knock_out_put", "worst_knock_out_call", "european_put", "european_call",
                      "asian_put_stderr", "asian_call_stderr", "knock_out_put_stderr", "knock_out_call_stderr",
                      "lookback_put_stderr", "lookback_call_stderr", "worst_knock_out_put_stderr",
                      "worst_knock_out_call_stderr", "european_put_stderr", "european_call_stderr", "mean_average",
                      "knocked_share", "worst_knocked_share", "mean_max", "mean_min")


@dataclass(frozen=True)
class BasketPathPrices:
    """``smc_basket_price_paths``'s block for B contracts: one [B] f64 device tensor per column (views of ``block``
    [B, 25], in ``BASKET_PATH_FIELDS`` order) and the raw terminal sums ``terminal_sum`` [B, A].  Knock-ins follow by
    difference: ``european_*`` minus ``knock_out_*``, and ``basket_price``'s ``worst_of_*`` minus
    ``worst_knock_out_*``."""
    asian_put: torch.Tensor
    asian_call: torch.Tensor
    knock_out_put: torch.Tensor
    knock_out_call: torch.Tensor
    lookback_put: torch.Tensor
    lookback_call: torch.Tensor
    worst_knock_out_put: torch.Tensor
    worst_knock_out_call: torch.Tensor
    european_put: torch.Tensor
    european_call: torch.Tensor
    asian_put_stderr: torch.Tensor
    asian_call_stderr: torch.Tensor
    knock_out_put_stderr: torch.Tensor
    knock_out_call_stderr: torch.Tensor
    lookback_put_stderr: torch.Tensor
    lookback_call_stderr: torch.Tensor
    worst_knock_out_put_stderr: torch.Tensor
    worst_knock_out_call_stderr: torch.Tensor
    european_put_stderr: torch.Tensor
    european_call_stderr: torch.Tensor
    mean_average: torch.Tensor
    knocked_share: torch.Tensor
    worst_knocked_share: torch.Tensor
    mean_max: torch.Tensor
    mean_min: torch.Tensor
    terminal_sum: torch.Tensor
    block: torch.Tensor


def validate_basket_barriers(barriers: torch.Tensor | None) -> None:
    """``basket_price_paths(validate=True)``'s checks of the barriers (they read the values): ValueError for a NaN
    and for a row with ``lower >= upper``."""
    if barriers is None:
        return
    if bool(torch.isnan(barriers).any()):
        raise ValueError("barriers must not be NaN (switch a side off with -inf / +inf)")
    if bool((barriers[:, 0] >= barriers[:, 1]).any()):
        raise ValueError("barriers must have lower < upper")


def basket_price_paths(contracts: torch.Tensor, cfg: BasketConfig, *, barriers: torch.Tensor | None = None,
                       weights: torch.Tensor | None = None, correlation: torch.Tensor | None = None,
                       ordinal0: int = 0, n_paths: int | None = None, validate: bool = False) -> BasketPathPrices:
    """Monte-Carlo prices of the path-dependent basket payoffs of device contracts [B, 3A+4] f64 (Asian, knock-out
    and lookback options on the weighted basket level, worst-of options knocked out on the worst asset, and the
    European basket beside them) over the ``cfg.timesteps`` monitoring dates: one launch of
    ``smc_basket_price_paths`` on the current stream, no host synchronisation.  ``cfg`` gives n_assets, timesteps,
    mc_seed, normalize and math; ``n_paths`` (default ``cfg.total_paths``) may be any positive count.

    ``barriers``: a contiguous float64 device tensor [B, 3] of (lower, upper, worst_lower) per contract: the basket
    is knocked out at a date where its level is <= lower or >= upper, the worst-of payoffs where the lowest scaled
    asset value is <= worst_lower.  A side is switched off with -inf / +inf (a spread's level may be negative, so 0
    is a level like any other); None switches all three off.  ``weights`` and ``correlation`` as ``basket_price``'s
    (None: 1 / A and the rows' rho).  ``validate=True`` checks the values first (``validate_basket_inputs``, and
    ``validate_basket_barriers``: no NaN, lower < upper) and is the only path that synchronises."""
    c = _batched_call(contracts, cfg, n_paths, weights, correlation, validate, barriers=barriers)
    B, A = c.B, c.A
    block = torch.empty((B, _lib.BASKET_PATH_COLS), dtype=torch.float64, device=contracts.device)
    tsum = torch.empty((B, A), dtype=torch.float64, device=contracts.device)
    if B > 0:
        _lib.check(_lib.lib().smc_basket_price_paths(
            _lib.ptr(contracts), _lib.ptr(c.weights), c.w_stride, _lib.ptr(c.tri), c.c_stride, _lib.ptr(barriers), B,
            A, cfg.timesteps, c.P, cfg.mc_seed, None, ordinal0, c.math, c.norm, _lib.ptr(block), _lib.ptr(tsum),
            _lib.stream_handle()))
    return BasketPathPrices(**{name: block[:, col] for col, name in enumerate(BASKET_PATH_FIELDS)}, terminal_sum=tsum,
                            block=block)

PATH_GREEK_PAYOFFS = ("asian_put", "asian_call", "lookback_put", "lookback_call")


def basket_path_greeks_fields(n_assets: int) -> tuple[str, ...]:
    """The names of ``smc_basket_greeks_paths``'s 16A + 24 columns in order.  Greek kinds ``delta_0`` ..
    ``delta_{A-1}``, ``vega_0`` .. ``vega_{A-1}``, ``rho``, ``theta``, each for the four payoffs of
    ``PATH_GREEK_PAYOFFS`` (``delta_asian_put_0``, ``delta_asian_call_0``, ``delta_lookback_put_0``, ...), the same
    names with ``_stderr``, the four prices and their ``_stderr``."""
    if not 1 <= n_assets <= MAX_ASSETS:
        raise ValueError(f"n_assets must be in 1..{MAX_ASSETS}, got {n_assets}")
    means = tuple(f"{kind}_{pay}_{i}" for kind in ("delta", "vega") for i in range(n_assets)
                  for pay in PATH_GREEK_PAYOFFS)
    means += tuple(f"{kind}_{pay}" for kind in ("rho", "theta") for pay in PATH_GREEK_PAYOFFS)
    return means + tuple(m + "_stderr" for m in means) + PATH_GREEK_PAYOFFS + tuple(
        p + "_stderr" for p in PATH_GREEK_PAYOFFS)


@dataclass(frozen=True)
class BasketPathGreeks:
    """``smc_basket_greeks_paths``'s block for B contracts of A assets.  Every field is a view of ``block``
    [B, 16A + 24] (``basket_path_greeks_fields`` order): per payoff of ``PATH_GREEK_PAYOFFS`` the per-asset ``delta_*``
    and ``vega_*`` [B, A], ``rho_*`` and ``theta_*`` (-dV/dT per year, every monitoring date moving with T) [B], their
    ``_stderr``, and the four prices with theirs (``smc_basket_price_paths``'s columns 0, 1, 4, 5 and 10, 11, 14, 15
    bit for bit)."""
    delta_asian_put: torch.Tensor
    delta_asian_call: torch.Tensor
    delta_lookback_put: torch.Tensor
    delta_lookback_call: torch.Tensor
    vega_asian_put: torch.Tensor
    vega_asian_call: torch.Tensor
    vega_lookback_put: torch.Tensor
    vega_lookback_call: torch.Tensor
    rho_asian_put: torch.Tensor
    rho_asian_call: torch.Tensor
    rho_lookback_put: torch.Tensor
    rho_lookback_call: torch.Tensor
    theta_asian_put: torch.Tensor
    theta_asian_call: torch.Tensor
    theta_lookback_put: torch.Tensor
    theta_lookback_call: torch.Tensor
    delta_asian_put_stderr: torch.Tensor
    delta_asian_call_stderr: torch.Tensor
    delta_lookback_put_stderr: torch.Tensor
    delta_lookback_call_stderr: torch.Tensor
    vega_asian_put_stderr: torch.Tensor
    vega_asian_call_stderr: torch.Tensor
    vega_lookback_put_stderr: torch.Tensor
    vega_lookback_call_stderr: torch.Tensor
    rho_asian_put_stderr: torch.Tensor
    rho_asian_call_stderr: torch.Tensor
    rho_lookback_put_stderr: torch.Tensor
    rho_lookback_call_stderr: torch.Tensor
    theta_asian_put_stderr: torch.Tensor
    theta_asian_call_stderr: torch.Tensor
    theta_lookback_put_stderr: torch.Tensor
    theta_lookback_call_stderr: torch.Tensor
    asian_put: torch.Tensor
    asian_call: torch.Tensor
    lookback_put: torch.Tensor
    lookback_call: torch.Tensor
    asian_put_stderr: torch.Tensor
    asian_call_stderr: torch.Tensor
    lookback_put_stderr: torch.Tensor
    lookback_call_stderr: torch.Tensor
    block: torch.Tensor


def _path_greeks_views(block: torch.Tensor, A: int) -> dict[str, torch.Tensor]:
    """The named views of a [B, 16A + 24] block (the column table of include/spectralmc_hip.h): Greek g of payoff q
    is column 4 g + q."""
    G = 2 * A + 2
    out: dict[str, torch.Tensor] = {}
    for suffix, base in (("", 0), ("_stderr", 4 * G)):
        for q, pay in enumerate(PATH_GREEK_PAYOFFS):
            out[f"delta_{pay}{suffix}"] = block[:, base + q:base + 4 * A:4]
            out[f"vega_{pay}{suffix}"] = block[:, base + 4 * A + q:base + 8 * A:4]
            out[f"rho_{pay}{suffix}"] = block[:, base + 8 * A + q]
            out[f"theta_{pay}{suffix}"] = block[:, base + 8 * A + 4 + q]
    for q, pay in enumerate(PATH_GREEK_PAYOFFS):
        out[pay] = block[:, 8 * G + q]
        out[pay + "_stderr"] = block[:, 8 * G + 4 + q]
    return out


def basket_greeks_paths(contracts: torch.Tensor, cfg: BasketConfig, *, weights: torch.Tensor | None = None,
                        correlation: torch.Tensor | None = None, ordinal0: int = 0, n_paths: int | None = None,
                        validate: bool = False) -> BasketPathGreeks:
    """Pathwise Greeks of the Asian and lookback basket options ``basket_price_paths`` prices, for device contracts
    [B, 3A+4] f64: per-asset deltas and vegas, rho and theta with standard errors and the four prices, in one launch
    of ``smc_basket_greeks_paths`` on the current stream, no host synchronisation.  ``cfg``, ``n_paths``, ``weights``
    and ``correlation`` as ``basket_price_paths``'s (there are no barriers: the knock-out payoffs have no pathwise
    Greeks).  ``validate=True`` checks the values first (``validate_basket_inputs``) and is the only path that
    synchronises."""
    c = _batched_call(contracts, cfg, n_paths, weights, correlation, validate)
    B, A = c.B, c.A
    block = torch.empty((B, _lib.basket_path_greeks_cols(A)), dtype=torch.float64, device=contracts.device)
    if B > 0:
        _lib.check(_lib.lib().smc_basket_greeks_paths(
            _lib.ptr(contracts), _lib.ptr(c.weights), c.w_stride, _lib.ptr(c.tri), c.c_stride, B, A, cfg.timesteps,
            c.P, cfg.mc_seed, None, ordinal0, c.math, c.norm, _lib.ptr(block), _lib.stream_handle()))
    return BasketPathGreeks(**_path_greeks_views(block, A), block=block)


def basket_greeks_fields(n_assets: int) -> tuple[str, ...]:
    """The names of ``smc_basket_greeks``'s 8A + 16 columns in order: per-asset ``delta_put_i``, ``delta_call_i``,
    ``vega_put_i``, ``vega_call_i``, then ``rho_put``, ``rho_call``, ``theta_*``, ``correlation_*``, the same names with
    ``_stderr``, and ``put``, ``call``, ``put_stderr``, ``call_stderr``."""
    if not 1 <= n_assets <= MAX_ASSETS:
        raise ValueError(f"n_assets must be in 1..{MAX_ASSETS}, got {n_assets}")
    means = tuple(f"{kind}_{side}_{i}" for kind in ("delta", "vega") for side in ("put", "call") for i in range(n_assets))
    means += tuple(f"{kind}_{side}" for kind in ("rho", "theta", "correlation") for side in ("put", "call"))
    return means + tuple(m + "_stderr" for m in means) + ("put", "call", "put_stderr", "call_stderr")


@dataclass(frozen=True)
class BasketGreeks:
    """``smc_basket_greeks``'s block for B contracts of A assets.  Every field but the three sums is a view of
    ``block`` [B, 8A + 16] (``basket_greeks_fields`` order): per-asset deltas and vegas [B, A], rho, theta (-dV/dT per
    year) and the sensitivity to the equicorrelation parameter [B], their standard errors, and the basket put and
    call prices with theirs (``smc_basket_price``'s columns 0, 1, 6, 7 bit for bit).  ``terminal_sum``, ``sum_xl``
    and ``sum_xc`` [B, A] are the pass-1 sums (the last two 0 under RAW)."""
    delta_put: torch.Tensor
    delta_call: torch.Tensor
    vega_put: torch.Tensor
    vega_call: torch.Tensor
    rho_put: torch.Tensor
    rho_call: torch.Tensor
    theta_put: torch.Tensor
    theta_call: torch.Tensor
    correlation_put: torch.Tensor
    correlation_call: torch.Tensor
    delta_put_stderr: torch.Tensor
    delta_call_stderr: torch.Tensor
    vega_put_stderr: torch.Tensor
    vega_call_stderr: torch.Tensor
    rho_put_stderr: torch.Tensor
    rho_call_stderr: torch.Tensor
    theta_put_stderr: torch.Tensor
    theta_call_stderr: torch.Tensor
    correlation_put_stderr: torch.Tensor
    correlation_call_stderr: torch.Tensor
    put: torch.Tensor
    call: torch.Tensor
    put_stderr: torch.Tensor
    call_stderr: torch.Tensor
    terminal_sum: torch.Tensor
    sum_xl: torch.Tensor
    sum_xc: torch.Tensor
    block: torch.Tensor


def _greeks_views(block: torch.Tensor, A: int) -> dict[str, torch.Tensor]:
    """The named views of a [B, 8A + 16] block (the column table of include/spectralmc_hip.h)."""
    n = 4 * A + 6
    out: dict[str, torch.Tensor] = {}
    for suffix, base in (("", 0), ("_stderr", n)):
        for j, name in enumerate(("delta_put", "delta_call", "vega_put", "vega_call")):
            out[name + suffix] = block[:, base + j * A:base + (j + 1) * A]
        for j, name in enumerate(("rho_put", "rho_call", "theta_put", "theta_call", "correlation_put",
                                  "correlation_call")):
            out[name + suffix] = block[:, base + 4 * A + j]
    for j, name in enumerate(("put", "call", "put_stderr", "call_stderr")):
        out[name] = block[:, 2 * n + j]
    return out


def basket_general_greeks_fields(n_assets: int) -> tuple[str, ...]:
    """The names of ``smc_basket_greeks_general``'s 2 A^2 + 6 A + 12 columns in order: ``basket_greeks_fields``'s with
    the two correlation columns replaced by one per pair in ``pack_correlation``'s order, ``correlation_put_j_k`` for
    every pair, then ``correlation_call_j_k``."""
    if not 1 <= n_assets <= MAX_ASSETS:
        raise ValueError(f"n_assets must be in 1..{MAX_ASSETS}, got {n_assets}")
    A = n_assets
    means = tuple(f"{kind}_{side}_{i}" for kind in ("delta", "vega") for side in ("put", "call") for i in range(A))
    means += tuple(f"{kind}_{side}" for kind in ("rho", "theta") for side in ("put", "call"))
    means += tuple(f"correlation_{side}_{j}_{k}" for side in ("put", "call") for j in range(A) for k in range(j))
    return means + tuple(m + "_stderr" for m in means) + ("put", "call", "put_stderr", "call_stderr")


@dataclass(frozen=True)
class BasketGeneralGreeks:
    """``smc_basket_greeks_general``'s block for B contracts of A assets with the caller's weights and correlation.
    Every field but the sums is a view of ``block`` [B, 2 A^2 + 6 A + 12] (``basket_general_greeks_fields`` order):
    ``BasketGreeks``'s fields, except that ``correlation_put`` / ``correlation_call`` and their ``_stderr`` are
    [B, A (A - 1) / 2], the sensitivity to each pair C_jk = C_kj in ``pack_correlation``'s order
    (``unpack_correlation`` gives the matrix form).  The prices are ``smc_basket_price_general``'s columns 0, 1, 6, 7
    bit for bit.  ``terminal_sum`` [B, A] and ``sum_moments`` [B, A (A + 1) / 2] (sum_p x_i ln(x_m / X0_m), m <= i, row
    by row; 0 under RAW) are the pass-1 sums."""
    delta_put: torch.Tensor
    delta_call: torch.Tensor
    vega_put: torch.Tensor
    vega_call: torch.Tensor
    rho_put: torch.Tensor
    rho_call: torch.Tensor
    theta_put: torch.Tensor
    theta_call: torch.Tensor
    correlation_put: torch.Tensor
    correlation_call: torch.Tensor
    delta_put_stderr: torch.Tensor
    delta_call_stderr: torch.Tensor
    vega_put_stderr: torch.Tensor
    vega_call_stderr: torch.Tensor
    rho_put_stderr: torch.Tensor
    rho_call_stderr: torch.Tensor
    theta_put_stderr: torch.Tensor
    theta_call_stderr: torch.Tensor
    correlation_put_stderr: torch.Tensor
    correlation_call_stderr: torch.Tensor
    put: torch.Tensor
    call: torch.Tensor
    put_stderr: torch.Tensor
    call_stderr: torch.Tensor
    terminal_sum: torch.Tensor
    sum_moments: torch.Tensor
    block: torch.Tensor


def _general_greeks_views(block: torch.Tensor, A: int) -> dict[str, torch.Tensor]:
    """The named views of a [B, 2 A^2 + 6 A + 12] block (the column table of include/spectralmc_hip.h)."""
    npairs = A * (A - 1) // 2
    n = 4 * A + 4 + 2 * npairs
    out: dict[str, torch.Tensor] = {}
    for suffix, base in (("", 0), ("_stderr", n)):
        for j, name in enumerate(("delta_put", "delta_call", "vega_put", "vega_call")):
            out[name + suffix] = block[:, base + j * A:base + (j + 1) * A]
        for j, name in enumerate(("rho_put", "rho_call", "theta_put", "theta_call")):
            out[name + suffix] = block[:, base + 4 * A + j]
        for j, name in enumerate(("correlation_put", "correlation_call")):
            out[name + suffix] = block[:, base + 4 * A + 4 + j * npairs:base + 4 * A + 4 + (j + 1) * npairs]
    for j, name in enumerate(("put", "call", "put_stderr", "call_stderr")):
        out[name] = block[:, 2 * n + j]
    return out


def basket_greeks(contracts: torch.Tensor, cfg: BasketConfig, *, ordinal0: int = 0, n_paths: int | None = None,
                  replay: bool = False, weights: torch.Tensor | None = None, correlation: torch.Tensor | None = None,
                  validate: bool = False) -> BasketGreeks | BasketGeneralGreeks:
    """Pathwise Greeks of the equal-weight basket put and call of device contracts [B, 3A+4] f64: one launch of
    ``smc_basket_greeks`` on the current stream, no host synchronisation.  Arguments as ``basket_price``.

    ``weights`` / ``correlation`` (either one given: one launch of ``smc_basket_greeks_general`` instead, returning
    ``BasketGeneralGreeks``): ``basket_price``'s arguments, with its meaning, shapes and checks.  The deltas and vegas
    are then those of the weighted basket (a negative weight flips their sign by itself) and the correlation
    sensitivity is reported per pair.  ``validate=True`` checks the values first (``validate_basket_inputs``) and is
    the only path that synchronises."""
    c = _batched_call(contracts, cfg, n_paths, weights, correlation, validate, replay=replay)
    B, A = c.B, c.A
    if c.general:
        block = torch.empty((B, _lib.basket_greeks_general_cols(A)), dtype=torch.float64, device=contracts.device)
        nm = A * (A + 1) // 2
        sums = torch.empty((B, A + nm), dtype=torch.float64, device=contracts.device)
        if B > 0:
            _lib.check(_lib.lib().smc_basket_greeks_general(
                _lib.ptr(contracts), _lib.ptr(c.weights), c.w_stride, _lib.ptr(c.tri), c.c_stride, B, A, cfg.timesteps,
                c.P, cfg.mc_seed, None, ordinal0, c.math, c.norm, _lib.ptr(block), _lib.ptr(sums),
                _lib.stream_handle()))
        return BasketGeneralGreeks(**_general_greeks_views(block, A), terminal_sum=sums[:, :A], sum_moments=sums[:, A:],
                                   block=block)
    block = torch.empty((B, _lib.basket_greeks_cols(A)), dtype=torch.float64, device=contracts.device)
    sums = torch.empty((B, 3, A), dtype=torch.float64, device=contracts.device)
    if B > 0:
        _lib.check(_lib.lib().smc_basket_greeks(
            _lib.ptr(contracts), B, A, cfg.timesteps, c.P, cfg.mc_seed, None, ordinal0, c.math, c.norm,
            _lib.ptr(block), _lib.ptr(sums), _lib.stream_handle()))
    return BasketGreeks(**_greeks_views(block, A), terminal_sum=sums[:, 0], sum_xl=sums[:, 1], sum_xc=sums[:, 2],
                        block=block)


class BasketEngine:
    """Device buffers + launches of the basket Monte-Carlo side of one training step
    (the ``TrainingEngine`` interface)."""

    def __init__(self, cfg: BasketConfig, batch_size: int, *, device: torch.device, sobol_skip: int = 0,
                 model_dtype: torch.dtype = torch.float32, rank: int = 0, world_size: int = 1,
                 store_paths: bool = True, path_buffer_bytes: int | None = None) -> None:
        _lib.require_device()
        self.cfg = cfg
        self.B = batch_size
        self.A = cfg.n_assets
        self.T = cfg.timesteps
        self.N = cfg.network_size
        self.M = cfg.batches_per_mc_run
        self.P = cfg.total_paths
        self.rank = rank
        self.world_size = world_size
        self.device = device
        self.dim = cfg.dim
        self._math = _lib.MATH_HW if cfg.math == "hw" else 0
        self.store_mode = _lib.STORE_ALL if store_paths else _lib.STORE_TERMINAL
        self._sobol = SobolEngine(self.dim, cfg.mc_seed, sobol_skip)
        lo, hi = cfg.arrays()
        self.tables = torch.from_numpy(self._sobol.tables().view("int32")).to(device)
        self.lower = torch.from_numpy(lo).to(device)
        self.upper = torch.from_numpy(hi).to(device)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=device)
        B = batch_size
        contracts = torch.empty((B, self.dim), dtype=torch.float64, device=device)
        real_in = torch.empty((B, self.dim), dtype=model_dtype, device=device)
        self.buffers = StepBuffers(contracts=contracts, real_in=real_in, imag_in=torch.zeros_like(real_in),
                                   targets=torch.empty((B, self.N), dtype=torch.complex64, device=device))
        self.terminal_sum = torch.empty((B, self.A), dtype=torch.float64, device=device)
        self.pitch = int(_lib.lib().smc_path_pitch(self.P, 0))
        rows = self.T if store_paths else 1
        per_contract = self.A * rows * self.pitch * 4
        budget = path_buffer_bytes if path_buffer_bytes is not None else _engine.path_buffer_budget(device)
        max_chunk = max(1, min(B, budget // per_contract))
        if max_chunk < B:
            # several launches: whole rounds of resident workgroups, so no launch ends in a
            # part-filled round (C5: 1171 -> 1024 contracts per launch, 2 full rounds each)
            slots = int(_lib.lib().smc_basket_resident_slots(self.A, self.N, self._math))
            if 0 < slots <= max_chunk:
                max_chunk -= max_chunk % slots
        launches = -(-B // max_chunk)
        self.chunk = -(-B // launches)  # equal launches
        shape = (self.chunk, self.A, rows, self.pitch)
        self._paths_buf = torch.empty(shape, dtype=torch.float32, device=device)
        self.paths = self._paths_buf[..., :self.P]
        self._f32_in = model_dtype == torch.float32
        # sync area of the resident kernel (zero-filled once; every launch leaves its counters zeroed);
        # the engine keeps the terminal sums, so other shapes run the split pair (simulate, then CF)
        self._sync_bytes = sync_bytes(cfg, self.chunk)
        self._sync = torch.zeros(self._sync_bytes, dtype=torch.uint8, device=device) if self._sync_bytes else None
        self.kernel_name = _lib.lib().smc_basket_train_targets_kernel(
            self.A, self.T, self.N, self.M, 1 if self._sync is not None else 0, 1).decode()

    @property
    def exchanges(self) -> bool:
        """The step's path launch has workgroups that wait for each other (the resident basket kernel)."""
        return self.kernel_name == "basket_resident_kernel"

    def check_status(self, stream: torch.cuda.Stream | None = None) -> None:
        """SmcError(SMC_ERR_EXCHANGE_TIMEOUT) if a resident launch gave up on a partner slice since the
        last check (engine.check_sync_status)."""
        check_sync_status(self._sync, stream)

    @property
    def global_batch(self) -> int:
        return self.B * self.world_size

    def algorithmic_bytes_per_contract(self) -> int:
        rows = self.T if self.store_mode == _lib.STORE_ALL else 1
        return self.A * rows * self.P * 4 + self.A * self.P * 4 + self.N * 8 + self.dim * 8

    def set_position(self, sobol_index: int, ordinal: int) -> None:
        self.cursor.copy_(torch.tensor([sobol_index, ordinal], dtype=torch.int64), non_blocking=False)

    def make_slot(self) -> StepBuffers:
        """Another set of step outputs (see TrainingEngine.make_slot)."""
        b = self.buffers
        return StepBuffers(contracts=torch.empty_like(b.contracts), real_in=torch.empty_like(b.real_in),
                           imag_in=b.imag_in, targets=torch.empty_like(b.targets))

    def enqueue_step(self, out: StepBuffers | None = None) -> StepBuffers:
        b = out if out is not None else self.buffers
        offset = self.rank * self.B
        draw_device(self.tables, self.dim, self.cursor[0:1], offset, self.B, self.lower, self.upper, b.contracts,
                    b.real_in if self._f32_in else None)
        if not self._f32_in:
            b.real_in.copy_(b.contracts)
        self.launch_targets(_lib.stream_handle(), _lib.ptr(self.cursor[1:2]), offset, b)
        self.cursor.add_(self.global_batch)
        return b

    def launch_targets(self, stream: int | None, ordinal_ptr: int | None, ordinal0: int,
                       b: StepBuffers | None = None) -> None:
        b = b if b is not None else self.buffers
        _lib.check(_lib.lib().smc_basket_train_targets(
            _lib.ptr(b.contracts), self.B, self.A, self.T, self.N, self.M, self.cfg.mc_seed, ordinal_ptr, ordinal0,
            self._math, 1 if self.cfg.normalize else 0, self.store_mode, _lib.ptr(self._paths_buf), self.pitch,
            self.chunk, _lib.ptr(self.terminal_sum), _lib.ptr(b.targets), _lib.ptr(self._sync), self._sync_bytes,
            stream))

    def price(self, contracts: torch.Tensor | None = None, *, ordinal0: int = 0,
              n_paths: int | None = None, weights: torch.Tensor | None = None,
              correlation: torch.Tensor | None = None) -> BasketPrices:
        """Monte-Carlo prices (``basket_price``) with the engine's configuration, by default of the contracts
        of the last enqueued step: the Monte-Carlo side of checking a basket-trained network.  ``weights`` and
        ``correlation`` as ``basket_price``'s (the training targets themselves stay equal-weight and
        equicorrelated)."""
        return basket_price(self.buffers.contracts if contracts is None else contracts, self.cfg, ordinal0=ordinal0,
                            n_paths=n_paths, weights=weights, correlation=correlation)

    def greeks(self, contracts: torch.Tensor | None = None, *, ordinal0: int = 0,
               n_paths: int | None = None, weights: torch.Tensor | None = None,
               correlation: torch.Tensor | None = None, validate: bool = False) -> BasketGreeks | BasketGeneralGreeks:
        """Pathwise Greeks (``basket_greeks``) with the engine's configuration, by default of the contracts of the
        last enqueued step.  ``weights``, ``correlation`` and ``validate`` as ``basket_greeks``'s."""
        return basket_greeks(self.buffers.contracts if contracts is None else contracts, self.cfg, ordinal0=ordinal0,
                             n_paths=n_paths, weights=weights, correlation=correlation, validate=validate)


    def price_paths(self, contracts: torch.Tensor | None = None, *, barriers: torch.Tensor | None = None,
                    weights: torch.Tensor | None = None, correlation: torch.Tensor | None = None, ordinal0: int = 0,
                    n_paths: int | None = None, validate: bool = False) -> BasketPathPrices:
        """Path-dependent Monte-Carlo prices (``basket_price_paths``) with the engine's configuration, by default of
        the contracts of the last enqueued step.  The other arguments as ``basket_price_paths``'s."""
        return basket_price_paths(self.buffers.contracts if contracts is None else contracts, self.cfg,
                                  barriers=barriers, weights=weights, correlation=correlation, ordinal0=ordinal0,
                                  n_paths=n_paths, validate=validate)

    def greeks_paths(self, contracts: torch.Tensor | None = None, *, weights: torch.Tensor | None = None,
                     correlation: torch.Tensor | None = None, ordinal0: int = 0, n_paths: int | None = None,
                     validate: bool = False) -> BasketPathGreeks:
        """Pathwise Greeks of the Asian and lookback basket options (``basket_greeks_paths``) with the engine's
        configuration, by default of the contracts of the last enqueued step.  The other arguments as
        ``basket_greeks_paths``'s."""
        return basket_greeks_paths(self.buffers.contracts if contracts is None else contracts, self.cfg,
                                   weights=weights, correlation=correlation, ordinal0=ordinal0, n_paths=n_paths,
                                   validate=validate)


def use_basket_engine(pricer, cfg: BasketConfig, *, store_paths: bool = True) -> None:
    """Make ``pricer`` train on basket contracts: its training sessions build a ``BasketEngine``
    instead of the single-asset engine.  The pricer's CVNN must take ``cfg.dim`` inputs."""
    def factory(p, batch_size: int, device: torch.device, rank: int, world_size: int) -> BasketEngine:
        return BasketEngine(cfg, batch_size, device=device, sobol_skip=0, model_dtype=p._dtype.to_torch(), rank=rank,
                            world_size=world_size, store_paths=store_paths)

    pricer.mc_engine_factory = factory


__all__ = ["BASKET_PATH_FIELDS", "PATH_GREEK_PAYOFFS", "BasketConfig", "BasketEngine", "BasketGeneralGreeks",
           "BasketGreeks", "BasketPathGreeks", "BasketPathPrices", "BasketPrices", "basket_fields",
           "basket_general_greeks_fields", "basket_greeks", "basket_greeks_fields", "basket_greeks_paths",
           "basket_path_greeks_fields", "basket_price", "basket_price_paths", "basket_targets", "default_basket_bounds", "pack_correlation",
           "unpack_correlation", "use_basket_engine", "validate_basket_barriers", "validate_basket_inputs", "MAX_ASSETS"]
