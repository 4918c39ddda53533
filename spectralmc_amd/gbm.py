"""GBM Monte-Carlo engine API (reference ``src/spectralmc/gbm.py``), backed by the HIP engine.

Public names and semantics follow the reference: ``SimulationParams`` /
``BlackScholesConfig`` + their ``build_*`` validators, and the single-GPU engine
``BlackScholes`` with ``_simulate`` -> ``price`` -> ``price_to_host`` and ``snapshot``.
``price_batch`` / ``price_batch_device`` (not in the reference) price many contracts in one
launch of the fused pricing kernel (``smc_gbm_price``); ``price_paths_batch`` /
``price_paths_batch_device`` do the same for the path-dependent payoffs (average-price, knock-out,
fixed-strike lookback) monitored at the time grid (``smc_gbm_price_paths``); ``greeks_batch`` /
``greeks_batch_device`` give the pathwise Greeks of the European pair on the same paths (``smc_gbm_greeks``).

What changed underneath:
* the normal matrix of contract m is not materialised: ``smc_gbm_simulate`` draws it in
  registers from the counter stream (mc_seed, m, path);
* ``SimulateBlackScholes`` (Numba, gbm.py:224-257) is the HIP path kernel, which also
  returns the per-row sums, so forward normalisation (gbm.py:435-438) is one in-place
  scaling pass (``smc_gbm_normalize``) instead of a mean pass plus a scaling pass;
* ``threads_per_block`` is validated as before but the HIP kernels choose their own
  geometry (wave64, 512-thread workgroups);
* device arrays are torch tensors on the process's GPU, all work on the current stream.
"""

from __future__ import annotations

from math import exp
from typing import Annotated, Literal, Sequence, TypeAlias

import numpy as np
import torch
from pydantic import BaseModel, ConfigDict, Field

from . import _lib
from .effects import ForwardNormalization, PathScheme
from .errors.async_normals import InvalidShape
from .errors.gbm import (
    GPUMemoryLimitExceeded,
    InvalidBlackScholesConfig,
    InvalidSimulationParams,
    NormalsGenerationFailed,
    NormalsUnavailable,
)
from .models.numerical import Precision
from .result import Failure, Result, Success
from .validation import validate_model

PosFloat = Annotated[float, Field(gt=0)]
NonNegFloat = Annotated[float, Field(ge=0)]
ThreadsPerBlock: TypeAlias = Literal[32, 64, 128, 256, 512, 1024]
NormalsError: TypeAlias = NormalsUnavailable | NormalsGenerationFailed

FIELDS: tuple[str, ...] = ("X0", "K", "T", "r", "d", "v")


class SimulationParams(BaseModel):
    """Immutable run-time parameters of one engine instance (reference gbm.py:77-103)."""

    timesteps: int = Field(..., gt=0)
    network_size: int = Field(..., gt=0)
    batches_per_mc_run: int = Field(..., gt=0)
    threads_per_block: ThreadsPerBlock
    mc_seed: int = Field(..., gt=0)
    buffer_size: int = Field(..., gt=0)
    skip: int = Field(0, ge=0)
    dtype: Precision

    model_config = ConfigDict(frozen=True, extra="forbid")

    def total_paths(self) -> int:
        return self.network_size * self.batches_per_mc_run

    def total_blocks(self) -> int:
        return (self.total_paths() + self.threads_per_block - 1) // self.threads_per_block


def validate_simulation_params_memory(params: SimulationParams) -> Result[SimulationParams, GPUMemoryLimitExceeded]:
    """Soft path-count guard (reference gbm.py:106-137)."""
    total = params.network_size * params.batches_per_mc_run
    limit = 1_000_000_000 if params.dtype == Precision.float32 else 500_000_000
    if total > limit:
        return Failure(GPUMemoryLimitExceeded(total_paths=total, max_paths=limit, network_size=params.network_size,
                                              batches_per_mc_run=params.batches_per_mc_run))
    return Success(params)


class BlackScholesConfig(BaseModel):
    sim_params: SimulationParams
    path_scheme: PathScheme = PathScheme.LOG_EULER
    normalization: ForwardNormalization = ForwardNormalization.NORMALIZE

    model_config = ConfigDict(frozen=True, extra="forbid")


def build_simulation_params(*, timesteps: int, network_size: int, batches_per_mc_run: int,
                            threads_per_block: ThreadsPerBlock, mc_seed: int, buffer_size: int, dtype: Precision,
                            skip: int = 0) -> Result[SimulationParams, InvalidSimulationParams | GPUMemoryLimitExceeded]:
    res = validate_model(SimulationParams, timesteps=timesteps, network_size=network_size,
                         batches_per_mc_run=batches_per_mc_run, threads_per_block=threads_per_block,
                         mc_seed=mc_seed, buffer_size=buffer_size, skip=skip, dtype=dtype)
    if isinstance(res, Failure):
        return Failure(InvalidSimulationParams(error=res.error))
    return validate_simulation_params_memory(res.value)


def build_black_scholes_config(*, sim_params: SimulationParams, path_scheme: PathScheme = PathScheme.LOG_EULER,
                               normalization: ForwardNormalization = ForwardNormalization.NORMALIZE
                               ) -> Result[BlackScholesConfig, InvalidBlackScholesConfig]:
    res = validate_model(BlackScholesConfig, sim_params=sim_params, path_scheme=path_scheme,
                         normalization=normalization)
    if isinstance(res, Failure):
        return Failure(InvalidBlackScholesConfig(error=res.error))
    return res


def scheme_code(scheme: PathScheme) -> int:
    return _lib.SCHEME_LOG_EULER if scheme is PathScheme.LOG_EULER else _lib.SCHEME_SIMPLE_EULER


def normalization_code(norm: ForwardNormalization) -> int:
    return _lib.NORM_NORMALIZE if norm is ForwardNormalization.NORMALIZE else _lib.NORM_RAW


def dtype_code(p: Precision) -> int:
    if p == Precision.float32:
        return _lib.DTYPE_F32
    if p == Precision.float64:
        return _lib.DTYPE_F64
    raise ValueError(f"simulation dtype must be float32 or float64, got {p}")


def time_grid(maturity: float, timesteps: int) -> np.ndarray:
    """``cp.linspace(dt, T, timesteps)`` evaluated in f64 (gbm.py:429), last point exact."""
    return np.linspace(maturity / timesteps, maturity, timesteps, dtype=np.float64)


class BlackScholes:
    """Single-GPU Monte-Carlo pricing engine (one process = one GPU)."""

    class Inputs(BaseModel):
        """One European option contract (reference gbm.py:267-277)."""

        X0: PosFloat
        K: PosFloat
        T: NonNegFloat
        r: float
        d: float
        v: NonNegFloat

        model_config = ConfigDict(frozen=True, extra="forbid")

    class SimResults(BaseModel):
        model_config = ConfigDict(arbitrary_types_allowed=True, extra="forbid")
        times: torch.Tensor
        sims: torch.Tensor
        forwards: torch.Tensor
        df: torch.Tensor

    class PricingResults(BaseModel):
        model_config = ConfigDict(arbitrary_types_allowed=True, extra="forbid")
        put_price_intrinsic: torch.Tensor
        call_price_intrinsic: torch.Tensor
        underlying: torch.Tensor
        put_price: torch.Tensor
        call_price: torch.Tensor

    class HostPricingResults(BaseModel):
        put_price_intrinsic: float
        call_price_intrinsic: float
        underlying: float
        put_convexity: float
        call_convexity: float
        put_price: float
        call_price: float

        model_config = ConfigDict(frozen=True, extra="forbid")

    class BatchPrices(BaseModel):
        """``smc_gbm_price``'s block for B contracts, column by column: ``[B]`` f64 device tensors."""

        model_config = ConfigDict(arbitrary_types_allowed=True, extra="forbid")
        put_price: torch.Tensor
        call_price: torch.Tensor
        underlying: torch.Tensor
        put_stderr: torch.Tensor
        call_stderr: torch.Tensor
        put_price_intrinsic: torch.Tensor
        call_price_intrinsic: torch.Tensor
        terminal_sum: torch.Tensor

    class PathBatchPrices(BaseModel):
        """``smc_gbm_price_paths``' block for B contracts, column by column: ``[B]`` f64 device tensors."""

        model_config = ConfigDict(arbitrary_types_allowed=True, extra="forbid")
        asian_put: torch.Tensor
        asian_call: torch.Tensor
        knock_out_put: torch.Tensor
        knock_out_call: torch.Tensor
        lookback_put: torch.Tensor
        lookback_call: torch.Tensor
        put_price: torch.Tensor
        call_price: torch.Tensor
        asian_put_stderr: torch.Tensor
        asian_call_stderr: torch.Tensor
        knock_out_put_stderr: torch.Tensor
        knock_out_call_stderr: torch.Tensor
        lookback_put_stderr: torch.Tensor
        lookback_call_stderr: torch.Tensor
        put_price_stderr: torch.Tensor
        call_price_stderr: torch.Tensor
        mean_average: torch.Tensor
        knocked_share: torch.Tensor
        mean_max: torch.Tensor
        mean_min: torch.Tensor

    class HostPathPrices(BaseModel):
        """One contract's row of ``PathBatchPrices`` on the host, with the knock-in prices (the European
        price minus the knock-out price)."""

        asian_put: float
        asian_call: float
        knock_out_put: float
        knock_out_call: float
        lookback_put: float
        lookback_call: float
        put_price: float
        call_price: float
        asian_put_stderr: float
        asian_call_stderr: float
        knock_out_put_stderr: float
        knock_out_call_stderr: float
        lookback_put_stderr: float
        lookback_call_stderr: float
        put_price_stderr: float
        call_price_stderr: float
        mean_average: float
        knocked_share: float
        mean_max: float
        mean_min: float
        knock_in_put: float
        knock_in_call: float

        model_config = ConfigDict(frozen=True, extra="forbid")

    class BatchGreeks(BaseModel):
        """``smc_gbm_greeks``' block for B contracts, column by column: ``[B]`` f64 device tensors (pathwise
        delta, vega, rho, theta = -dV/dT per year, gamma from the lognormal identity; their standard errors; the
        prices ``price_batch_device`` gives on the same paths; the two terminal sums)."""

        model_config = ConfigDict(arbitrary_types_allowed=True, extra="forbid")
        put_delta: torch.Tensor
        call_delta: torch.Tensor
        put_vega: torch.Tensor
        call_vega: torch.Tensor
        put_rho: torch.Tensor
        call_rho: torch.Tensor
        put_theta: torch.Tensor
        call_theta: torch.Tensor
        put_gamma: torch.Tensor
        call_gamma: torch.Tensor
        put_delta_stderr: torch.Tensor
        call_delta_stderr: torch.Tensor
        put_vega_stderr: torch.Tensor
        call_vega_stderr: torch.Tensor
        put_rho_stderr: torch.Tensor
        call_rho_stderr: torch.Tensor
        put_theta_stderr: torch.Tensor
        call_theta_stderr: torch.Tensor
        put_gamma_stderr: torch.Tensor
        call_gamma_stderr: torch.Tensor
        put_price: torch.Tensor
        call_price: torch.Tensor
        put_stderr: torch.Tensor
        call_stderr: torch.Tensor
        terminal_sum: torch.Tensor
        terminal_log_sum: torch.Tensor

    class HostGreeks(BaseModel):
        """One contract's row of ``BatchGreeks`` on the host."""

        put_delta: float
        call_delta: float
        put_vega: float
        call_vega: float
        put_rho: float
        call_rho: float
        put_theta: float
        call_theta: float
        put_gamma: float
        call_gamma: float
        put_delta_stderr: float
        call_delta_stderr: float
        put_vega_stderr: float
        call_vega_stderr: float
        put_rho_stderr: float
        call_rho_stderr: float
        put_theta_stderr: float
        call_theta_stderr: float
        put_gamma_stderr: float
        call_gamma_stderr: float
        put_price: float
        call_price: float
        put_stderr: float
        call_stderr: float
        terminal_sum: float
        terminal_log_sum: float

        model_config = ConfigDict(frozen=True, extra="forbid")

    class PathBatchGreeks(BaseModel):
        """``smc_gbm_greeks_paths``' block for B contracts, column by column: ``[B]`` f64 device tensors (pathwise
        delta, vega, rho and theta = -dV/dT per year of the Asian and lookback options, their standard errors, and the
        four prices ``price_paths_batch_device`` gives on the same paths with theirs)."""

        model_config = ConfigDict(arbitrary_types_allowed=True, extra="forbid")
        asian_put_delta: torch.Tensor
        asian_call_delta: torch.Tensor
        lookback_put_delta: torch.Tensor
        lookback_call_delta: torch.Tensor
        asian_put_vega: torch.Tensor
        asian_call_vega: torch.Tensor
        lookback_put_vega: torch.Tensor
        lookback_call_vega: torch.Tensor
        asian_put_rho: torch.Tensor
        asian_call_rho: torch.Tensor
        lookback_put_rho: torch.Tensor
        lookback_call_rho: torch.Tensor
        asian_put_theta: torch.Tensor
        asian_call_theta: torch.Tensor
        lookback_put_theta: torch.Tensor
        lookback_call_theta: torch.Tensor
        asian_put_delta_stderr: torch.Tensor
        asian_call_delta_stderr: torch.Tensor
        lookback_put_delta_stderr: torch.Tensor
        lookback_call_delta_stderr: torch.Tensor
        asian_put_vega_stderr: torch.Tensor
        asian_call_vega_stderr: torch.Tensor
        lookback_put_vega_stderr: torch.Tensor
        lookback_call_vega_stderr: torch.Tensor
        asian_put_rho_stderr: torch.Tensor
        asian_call_rho_stderr: torch.Tensor
        lookback_put_rho_stderr: torch.Tensor
        lookback_call_rho_stderr: torch.Tensor
        asian_put_theta_stderr: torch.Tensor
        asian_call_theta_stderr: torch.Tensor
        lookback_put_theta_stderr: torch.Tensor
        lookback_call_theta_stderr: torch.Tensor
        asian_put: torch.Tensor
        asian_call: torch.Tensor
        lookback_put: torch.Tensor
        lookback_call: torch.Tensor
        asian_put_stderr: torch.Tensor
        asian_call_stderr: torch.Tensor
        lookback_put_stderr: torch.Tensor
        lookback_call_stderr: torch.Tensor

    class HostPathGreeks(BaseModel):
        """One contract's row of ``PathBatchGreeks`` on the host."""

        asian_put_delta: float
        asian_call_delta: float
        lookback_put_delta: float
        lookback_call_delta: float
        asian_put_vega: float
        asian_call_vega: float
        lookback_put_vega: float
        lookback_call_vega: float
        asian_put_rho: float
        asian_call_rho: float
        lookback_put_rho: float
        lookback_call_rho: float
        asian_put_theta: float
        asian_call_theta: float
        lookback_put_theta: float
        lookback_call_theta: float
        asian_put_delta_stderr: float
        asian_call_delta_stderr: float
        lookback_put_delta_stderr: float
        lookback_call_delta_stderr: float
        asian_put_vega_stderr: float
        asian_call_vega_stderr: float
        lookback_put_vega_stderr: float
        lookback_call_vega_stderr: float
        asian_put_rho_stderr: float
        asian_call_rho_stderr: float
        lookback_put_rho_stderr: float
        lookback_call_rho_stderr: float
        asian_put_theta_stderr: float
        asian_call_theta_stderr: float
        lookback_put_theta_stderr: float
        lookback_call_theta_stderr: float
        asian_put: float
        asian_call: float
        lookback_put: float
        lookback_call: float
        asian_put_stderr: float
        asian_call_stderr: float
        lookback_put_stderr: float
        lookback_call_stderr: float

        model_config = ConfigDict(frozen=True, extra="forbid")

    #: path math of price_batch / price_batch_device and of price_paths_batch / price_paths_batch_device: "portable" (IEEE-only transcendentals, the draws and
    #: arithmetic of price / price_to_host) or "hw" (hardware f32 transcendentals, float32 engines only:
    #: throughput mode, within the f32 tolerance of "portable")
    price_batch_math: str = "portable"

    def __init__(self, cfg: BlackScholesConfig) -> None:
        self._cfg = cfg
        self._sp = cfg.sim_params
        self._torch_dtype = self._sp.dtype.to_torch()
        self._served = self._sp.skip  # normal matrices consumed so far (= next contract ordinal)
        # The reference validates the normal-buffer size against one matrix
        # (async_normals.py:112-125); an invalid size surfaces as NormalsUnavailable.
        sp = self._sp
        self._normals_error = (InvalidShape(rows=sp.timesteps, cols=sp.total_paths())
                               if sp.buffer_size > sp.timesteps * sp.total_paths() else None)

    # ------------------------------------------------------------------ state
    @property
    def config(self) -> BlackScholesConfig:
        return self._cfg

    @property
    def ordinal(self) -> int:
        """Ordinal of the next contract's normal stream (= matrices served)."""
        return self._served

    def advance(self, n: int) -> None:
        """Account for n contracts simulated by the fused trainer kernel."""
        self._served += n

    def snapshot(self) -> Result[BlackScholesConfig, NormalsUnavailable]:
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        sp = self._sp.model_copy(update={"skip": self._served}, deep=True)
        return Success(self._cfg.model_copy(update={"sim_params": sp}, deep=True))

    # ------------------------------------------------------------------ engine
    def _device(self) -> torch.device:
        _lib.require_device()
        return torch.device("cuda", torch.cuda.current_device())

    def _contract_tensor(self, inputs: "BlackScholes.Inputs", device: torch.device) -> torch.Tensor:
        row = [float(getattr(inputs, f)) for f in FIELDS]
        return torch.tensor([row], dtype=torch.float64, device=device)

    def _simulate(self, inputs: "BlackScholes.Inputs") -> Result["BlackScholes.SimResults", NormalsError]:
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        dev = self._device()
        sp = self._sp
        T, P = sp.timesteps, sp.total_paths()
        contract = self._contract_tensor(inputs, dev)
        sims = torch.empty((T, P), dtype=self._torch_dtype, device=dev)
        rowsum = torch.empty((1, T), dtype=torch.float64, device=dev)
        L = _lib.lib()
        stream = _lib.stream_handle()
        _lib.check(L.smc_gbm_simulate(_lib.ptr(contract), 1, T, P, sp.mc_seed, None, self._served,
                                      scheme_code(self._cfg.path_scheme), dtype_code(sp.dtype), _lib.ptr(sims),
                                      _lib.ptr(rowsum), stream))
        self._served += 1
        times = torch.tensor(time_grid(inputs.T, T), device=dev).to(self._torch_dtype)
        rate = torch.tensor(inputs.r - inputs.d, dtype=self._torch_dtype, device=dev)
        forwards = torch.tensor(inputs.X0, dtype=self._torch_dtype, device=dev) * torch.exp(rate * times)
        df = torch.exp(torch.tensor(-inputs.r, dtype=self._torch_dtype, device=dev) * times)
        if self._cfg.normalization is ForwardNormalization.NORMALIZE:
            _lib.check(L.smc_gbm_normalize(_lib.ptr(contract), 1, T, P, dtype_code(sp.dtype), _lib.ptr(sims),
                                           _lib.ptr(rowsum), stream))
        return Success(self.SimResults(times=times, sims=sims, forwards=forwards, df=df))

    def price(self, *, inputs: "BlackScholes.Inputs",
              sr_result: "Result[BlackScholes.SimResults, NormalsError] | None" = None
              ) -> Result["BlackScholes.PricingResults", NormalsError]:
        sim = sr_result or self._simulate(inputs)
        if isinstance(sim, Failure):
            return sim
        sr = sim.value
        F, df_last = sr.forwards[-1], sr.df[-1]
        K = torch.tensor(inputs.K, dtype=self._torch_dtype, device=sr.sims.device)
        terminal = sr.sims[-1]
        zero = torch.zeros((), dtype=self._torch_dtype, device=sr.sims.device)
        return Success(self.PricingResults(
            put_price_intrinsic=df_last * torch.maximum(K - F, zero),
            call_price_intrinsic=df_last * torch.maximum(F - K, zero),
            underlying=terminal,
            put_price=df_last * torch.maximum(K - terminal, zero),
            call_price=df_last * torch.maximum(terminal - K, zero),
        ))

    def get_host_price(self, pr: "BlackScholes.PricingResults") -> "BlackScholes.HostPricingResults":
        put_intr = float(pr.put_price_intrinsic.item())
        call_intr = float(pr.call_price_intrinsic.item())
        put = float(pr.put_price.mean().item())
        call = float(pr.call_price.mean().item())
        return self.HostPricingResults(put_price_intrinsic=put_intr, call_price_intrinsic=call_intr,
                                       underlying=float(pr.underlying.mean().item()),
                                       put_convexity=put - put_intr, call_convexity=call - call_intr,
                                       put_price=put, call_price=call)

    def price_to_host(self, inputs: "BlackScholes.Inputs") -> Result["BlackScholes.HostPricingResults", NormalsError]:
        res = self.price(inputs=inputs)
        if isinstance(res, Failure):
            return res
        return Success(self.get_host_price(res.value))

    # ------------------------------------------------------------------ batched pricing
    def _price_block(self, contracts: torch.Tensor) -> Result[torch.Tensor, NormalsError]:
        """One ``smc_gbm_price`` launch on the current stream (no sync): the ``[B, 8]`` f64 block of
        contracts ``[B, 6]`` f64 on the device; contract b takes ordinal ``ordinal + b``."""
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if contracts.ndim != 2 or contracts.shape[1] != len(FIELDS) or contracts.dtype != torch.float64:
            raise ValueError(f"contracts must be a [B, {len(FIELDS)}] float64 tensor, got "
                             f"{tuple(contracts.shape)} {contracts.dtype}")
        _lib.require_device()
        if not contracts.is_cuda:
            raise ValueError("contracts must be a device tensor")
        sp = self._sp
        contracts = contracts.contiguous()
        B = int(contracts.shape[0])
        block = torch.empty((B, _lib.PRICE_COLS), dtype=torch.float64, device=contracts.device)
        if self.price_batch_math not in ("portable", "hw"):
            raise ValueError(f"price_batch_math must be 'portable' or 'hw', got {self.price_batch_math!r}")
        scheme = scheme_code(self._cfg.path_scheme) | (_lib.MATH_HW if self.price_batch_math == "hw" else 0)
        if B:
            _lib.check(_lib.lib().smc_gbm_price(
                _lib.ptr(contracts), B, sp.timesteps, sp.total_paths(), sp.mc_seed, None, self._served,
                scheme, normalization_code(self._cfg.normalization), dtype_code(sp.dtype),
                _lib.ptr(block), _lib.stream_handle()))
            self._served += B
        return Success(block)

    def price_batch_device(self, contracts: torch.Tensor) -> Result["BlackScholes.BatchPrices", NormalsError]:
        """Monte-Carlo prices of B contracts (``[B, 6]`` f64 device tensor, columns X0 K T r d v) in one
        launch of the fused pricing kernel: no path matrix in memory, no host sync.  Consumes the
        normal streams of B ``price`` calls (``snapshot`` reflects it)."""
        res = self._price_block(contracts)
        if isinstance(res, Failure):
            return res
        put, call, und, put_se, call_se, put_in, call_in, tsum = res.value.unbind(dim=1)
        return Success(self.BatchPrices(put_price=put, call_price=call, underlying=und, put_stderr=put_se,
                                        call_stderr=call_se, put_price_intrinsic=put_in,
                                        call_price_intrinsic=call_in, terminal_sum=tsum))

    def price_batch(self, inputs: "Sequence[BlackScholes.Inputs]"
                    ) -> Result["list[BlackScholes.HostPricingResults]", NormalsError]:
        """``[price_to_host(c) for c in inputs]`` as one launch and one device-to-host copy."""
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if len(inputs) == 0:
            return Success([])
        rows = [[float(getattr(c, f)) for f in FIELDS] for c in inputs]
        res = self._price_block(torch.tensor(rows, dtype=torch.float64, device=self._device()))
        if isinstance(res, Failure):
            return res
        out = []
        for put, call, und, _, _, put_in, call_in, _ in res.value.cpu().tolist():
            out.append(self.HostPricingResults(put_price_intrinsic=put_in, call_price_intrinsic=call_in,
                                               underlying=und, put_convexity=put - put_in,
                                               call_convexity=call - call_in, put_price=put, call_price=call))
        return Success(out)

    # ------------------------------------------------------------------ sliced batched pricing
    def _price_sliced_block(self, contracts: torch.Tensor, slice_paths: int | None
                            ) -> Result[torch.Tensor, NormalsError]:
        """One ``smc_gbm_price_sliced`` call on the current stream (no sync): the ``[B, 8]`` f64 block of
        contracts ``[B, 6]`` f64 on the device, each contract cut into slices of ``slice_paths`` paths
        (``None``: ``smc_gbm_price_slice_paths``), one workgroup per slice; contract b takes ordinal
        ``ordinal + b``.  The workspace comes from the caching allocator."""
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if contracts.ndim != 2 or contracts.shape[1] != len(FIELDS) or contracts.dtype != torch.float64:
            raise ValueError(f"contracts must be a [B, {len(FIELDS)}] float64 tensor, got "
                             f"{tuple(contracts.shape)} {contracts.dtype}")
        _lib.require_device()
        if not contracts.is_cuda:
            raise ValueError("contracts must be a device tensor")
        sp = self._sp
        contracts = contracts.contiguous()
        B = int(contracts.shape[0])
        block = torch.empty((B, _lib.PRICE_COLS), dtype=torch.float64, device=contracts.device)
        if self.price_batch_math not in ("portable", "hw"):
            raise ValueError(f"price_batch_math must be 'portable' or 'hw', got {self.price_batch_math!r}")
        scheme = scheme_code(self._cfg.path_scheme) | (_lib.MATH_HW if self.price_batch_math == "hw" else 0)
        L = _lib.lib()
        P = sp.total_paths()
        span = int(L.smc_gbm_price_slice_paths(P)) if slice_paths is None else int(slice_paths)
        if B:
            nbytes = int(L.smc_gbm_price_sliced_workspace_bytes(B, P, span))
            if nbytes < 0:
                raise ValueError(f"slice_paths must be a positive multiple of 2048 that cuts {P} paths into at most "
                                 f"65,535 slices (fewer than 2^31 workgroups in all), got {span}")
            workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=contracts.device)
            _lib.check(L.smc_gbm_price_sliced(
                _lib.ptr(contracts), B, sp.timesteps, P, span, sp.mc_seed, None, self._served,
                scheme, normalization_code(self._cfg.normalization), dtype_code(sp.dtype),
                _lib.ptr(block), _lib.ptr(workspace), nbytes, _lib.stream_handle()))
            self._served += B
        return Success(block)

    def price_sliced_device(self, contracts: torch.Tensor, slice_paths: int | None = None
                            ) -> Result["BlackScholes.BatchPrices", NormalsError]:
        """``price_batch_device`` with every contract spread over ``ceil(P / slice_paths)`` workgroups: for one
        contract, or a few dozen, at a path count where one workgroup per contract leaves the chip idle.  Device
        tensors in and out, the current stream, no host sync.  With one slice the values are ``price_batch_device``'s
        replay-mode bits; with more, the f64 sums are added slice by slice and the last bits may differ."""
        res = self._price_sliced_block(contracts, slice_paths)
        if isinstance(res, Failure):
            return res
        put, call, und, put_se, call_se, put_in, call_in, tsum = res.value.unbind(dim=1)
        return Success(self.BatchPrices(put_price=put, call_price=call, underlying=und, put_stderr=put_se,
                                        call_stderr=call_se, put_price_intrinsic=put_in,
                                        call_price_intrinsic=call_in, terminal_sum=tsum))

    def price_sliced(self, inputs: "Sequence[BlackScholes.Inputs]", slice_paths: int | None = None
                     ) -> Result["list[BlackScholes.HostPricingResults]", NormalsError]:
        """``price_batch`` through the sliced call: one device-to-host copy."""
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if len(inputs) == 0:
            return Success([])
        rows = [[float(getattr(c, f)) for f in FIELDS] for c in inputs]
        res = self._price_sliced_block(torch.tensor(rows, dtype=torch.float64, device=self._device()), slice_paths)
        if isinstance(res, Failure):
            return res
        out = []
        for put, call, und, _, _, put_in, call_in, _ in res.value.cpu().tolist():
            out.append(self.HostPricingResults(put_price_intrinsic=put_in, call_price_intrinsic=call_in,
                                               underlying=und, put_convexity=put - put_in,
                                               call_convexity=call - call_in, put_price=put, call_price=call))
        return Success(out)

    # ------------------------------------------------------------------ batched path-dependent pricing
    def _path_price_block(self, contracts: torch.Tensor, barriers: torch.Tensor | None
                          ) -> Result[torch.Tensor, NormalsError]:
        """One ``smc_gbm_price_paths`` launch on the current stream (no sync): the ``[B, 20]`` f64 block of
        contracts ``[B, 6]`` (and barriers ``[B, 2]`` or None) f64 on the device; contract b takes ordinal
        ``ordinal + b``."""
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        for name, t, cols in (("contracts", contracts, len(FIELDS)), ("barriers", barriers, 2)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.ndim != 2 or t.shape[1] != cols or t.dtype != torch.float64:
                raise ValueError(f"{name} must be a [B, {cols}] float64 tensor, got "
                                 f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t))}")
        if barriers is not None and barriers.shape[0] != contracts.shape[0]:
            raise ValueError(f"barriers must have one (lower, upper) row per contract: {barriers.shape[0]} rows "
                             f"for {contracts.shape[0]} contracts")
        _lib.require_device()
        if not contracts.is_cuda or (barriers is not None and barriers.device != contracts.device):
            raise ValueError("contracts and barriers must be tensors on the same device")
        if self.price_batch_math not in ("portable", "hw"):
            raise ValueError(f"price_batch_math must be 'portable' or 'hw', got {self.price_batch_math!r}")
        sp = self._sp
        contracts = contracts.contiguous()
        barriers = None if barriers is None else barriers.contiguous()
        B = int(contracts.shape[0])
        block = torch.empty((B, _lib.PATH_PRICE_COLS), dtype=torch.float64, device=contracts.device)
        scheme = scheme_code(self._cfg.path_scheme) | (_lib.MATH_HW if self.price_batch_math == "hw" else 0)
        if B:
            _lib.check(_lib.lib().smc_gbm_price_paths(
                _lib.ptr(contracts), _lib.ptr(barriers), B, sp.timesteps, sp.total_paths(), sp.mc_seed, None,
                self._served, scheme, normalization_code(self._cfg.normalization), dtype_code(sp.dtype),
                _lib.ptr(block), _lib.stream_handle()))
            self._served += B
        return Success(block)

    def price_paths_batch_device(self, contracts: torch.Tensor, barriers: torch.Tensor | None = None
                                 ) -> Result["BlackScholes.PathBatchPrices", NormalsError]:
        """Path-dependent Monte-Carlo prices of B contracts (``[B, 6]`` f64 device tensor, columns X0 K T r d v)
        in one launch of the fused kernel, with no path matrix in memory and no host sync: average-price
        (Asian), knock-out and fixed-strike lookback puts and calls beside the European pair, monitored at
        the engine's ``timesteps`` grid points.  ``barriers`` is a ``[B, 2]`` f64 device tensor of
        (lower, upper) per contract, or None for no barrier.  Consumes the normal streams of B ``price``
        calls (``snapshot`` reflects it)."""
        res = self._path_price_block(contracts, barriers)
        if isinstance(res, Failure):
            return res
        return Success(self.PathBatchPrices(**dict(zip(self.PathBatchPrices.model_fields, res.value.unbind(dim=1)))))

    def price_paths_batch(self, inputs: "Sequence[BlackScholes.Inputs]",
                          barriers: "Sequence[tuple[float, float]] | None" = None
                          ) -> Result["list[BlackScholes.HostPathPrices]", NormalsError]:
        """``price_paths_batch_device`` from host values: one launch and one device-to-host copy.
        ``barriers`` is one (lower, upper) pair per contract, or None."""
        if barriers is not None and len(barriers) != len(inputs):
            raise ValueError(f"barriers must have one (lower, upper) pair per contract: {len(barriers)} pairs "
                             f"for {len(inputs)} contracts")
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if len(inputs) == 0:
            return Success([])
        dev = self._device()
        rows = [[float(getattr(c, f)) for f in FIELDS] for c in inputs]
        bars = None if barriers is None else torch.tensor([[float(lo), float(up)] for lo, up in barriers],
                                                          dtype=torch.float64, device=dev)
        res = self._path_price_block(torch.tensor(rows, dtype=torch.float64, device=dev), bars)
        if isinstance(res, Failure):
            return res
        names = list(self.PathBatchPrices.model_fields)
        out = []
        for row in res.value.cpu().tolist():
            cols = dict(zip(names, row))
            out.append(self.HostPathPrices(knock_in_put=cols["put_price"] - cols["knock_out_put"],
                                           knock_in_call=cols["call_price"] - cols["knock_out_call"], **cols))
        return Success(out)

    # ------------------------------------------------------------------ batched Greeks
    def _greeks_block(self, contracts: torch.Tensor) -> Result[torch.Tensor, NormalsError]:
        """One ``smc_gbm_greeks`` launch on the current stream (no sync): the ``[B, 26]`` f64 block of
        contracts ``[B, 6]`` f64 on the device; contract b takes ordinal ``ordinal + b``."""
        if self._cfg.path_scheme is not PathScheme.LOG_EULER:
            raise ValueError(f"greeks_batch needs PathScheme.LOG_EULER, got {self._cfg.path_scheme.name}: the pathwise "
                             "Greeks are functions of the log-Euler terminal value")
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if contracts.ndim != 2 or contracts.shape[1] != len(FIELDS) or contracts.dtype != torch.float64:
            raise ValueError(f"contracts must be a [B, {len(FIELDS)}] float64 tensor, got "
                             f"{tuple(contracts.shape)} {contracts.dtype}")
        _lib.require_device()
        if not contracts.is_cuda:
            raise ValueError("contracts must be a device tensor")
        sp = self._sp
        contracts = contracts.contiguous()
        B = int(contracts.shape[0])
        block = torch.empty((B, _lib.GREEKS_COLS), dtype=torch.float64, device=contracts.device)
        if self.price_batch_math not in ("portable", "hw"):
            raise ValueError(f"price_batch_math must be 'portable' or 'hw', got {self.price_batch_math!r}")
        scheme = scheme_code(self._cfg.path_scheme) | (_lib.MATH_HW if self.price_batch_math == "hw" else 0)
        if B:
            _lib.check(_lib.lib().smc_gbm_greeks(
                _lib.ptr(contracts), B, sp.timesteps, sp.total_paths(), sp.mc_seed, None, self._served,
                scheme, normalization_code(self._cfg.normalization), dtype_code(sp.dtype),
                _lib.ptr(block), _lib.stream_handle()))
            self._served += B
        return Success(block)

    def greeks_batch_device(self, contracts: torch.Tensor) -> Result["BlackScholes.BatchGreeks", NormalsError]:
        """Pathwise Greeks of the European put and call of B contracts (``[B, 6]`` f64 device tensor, columns
        X0 K T r d v) in one launch of the fused kernel, with no path matrix in memory and no host sync: the
        derivatives of the estimator ``price_batch_device`` computes, on the same paths, with their standard
        errors.  LOG_EULER engines only.  Consumes the normal streams of B ``price`` calls."""
        res = self._greeks_block(contracts)
        if isinstance(res, Failure):
            return res
        return Success(self.BatchGreeks(**dict(zip(self.BatchGreeks.model_fields, res.value.unbind(dim=1)))))

    def greeks_batch(self, inputs: "Sequence[BlackScholes.Inputs]"
                     ) -> Result["list[BlackScholes.HostGreeks]", NormalsError]:
        """``greeks_batch_device`` from host values: one launch and one device-to-host copy."""
        if self._cfg.path_scheme is not PathScheme.LOG_EULER:
            raise ValueError(f"greeks_batch needs PathScheme.LOG_EULER, got {self._cfg.path_scheme.name}: the pathwise "
                             "Greeks are functions of the log-Euler terminal value")
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if len(inputs) == 0:
            return Success([])
        rows = [[float(getattr(c, f)) for f in FIELDS] for c in inputs]
        res = self._greeks_block(torch.tensor(rows, dtype=torch.float64, device=self._device()))
        if isinstance(res, Failure):
            return res
        names = list(self.BatchGreeks.model_fields)
        return Success([self.HostGreeks(**dict(zip(names, row))) for row in res.value.cpu().tolist()])

    # ------------------------------------------------------------------ sliced batched Greeks
    def _greeks_sliced_block(self, contracts: torch.Tensor, slice_paths: int | None
                             ) -> Result[torch.Tensor, NormalsError]:
        """One ``smc_gbm_greeks_sliced`` call on the current stream (no sync): the ``[B, 26]`` f64 block of
        contracts ``[B, 6]`` f64 on the device, each contract cut into slices of ``slice_paths`` paths
        (``None``: ``smc_gbm_price_slice_paths``, the price call's rule), one workgroup per slice; contract b
        takes ordinal ``ordinal + b``.  The workspace comes from the caching allocator."""
        if self._cfg.path_scheme is not PathScheme.LOG_EULER:
            raise ValueError(f"greeks_sliced needs PathScheme.LOG_EULER, got {self._cfg.path_scheme.name}: the pathwise "
                             "Greeks are functions of the log-Euler terminal value")
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if contracts.ndim != 2 or contracts.shape[1] != len(FIELDS) or contracts.dtype != torch.float64:
            raise ValueError(f"contracts must be a [B, {len(FIELDS)}] float64 tensor, got "
                             f"{tuple(contracts.shape)} {contracts.dtype}")
        _lib.require_device()
        if not contracts.is_cuda:
            raise ValueError("contracts must be a device tensor")
        sp = self._sp
        contracts = contracts.contiguous()
        B = int(contracts.shape[0])
        block = torch.empty((B, _lib.GREEKS_COLS), dtype=torch.float64, device=contracts.device)
        if self.price_batch_math not in ("portable", "hw"):
            raise ValueError(f"price_batch_math must be 'portable' or 'hw', got {self.price_batch_math!r}")
        scheme = scheme_code(self._cfg.path_scheme) | (_lib.MATH_HW if self.price_batch_math == "hw" else 0)
        L = _lib.lib()
        P = sp.total_paths()
        span = int(L.smc_gbm_price_slice_paths(P)) if slice_paths is None else int(slice_paths)
        if B:
            nbytes = int(L.smc_gbm_greeks_sliced_workspace_bytes(B, P, span))
            if nbytes < 0:
                raise ValueError(f"slice_paths must be a positive multiple of 2048 that cuts {P} paths into at most "
                                 f"65,535 slices (fewer than 2^31 workgroups in all), got {span}")
            workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=contracts.device)
            _lib.check(L.smc_gbm_greeks_sliced(
                _lib.ptr(contracts), B, sp.timesteps, P, span, sp.mc_seed, None, self._served,
                scheme, normalization_code(self._cfg.normalization), dtype_code(sp.dtype),
                _lib.ptr(block), _lib.ptr(workspace), nbytes, _lib.stream_handle()))
            self._served += B
        return Success(block)

    def greeks_sliced_device(self, contracts: torch.Tensor, slice_paths: int | None = None
                             ) -> Result["BlackScholes.BatchGreeks", NormalsError]:
        """``greeks_batch_device`` with every contract spread over ``ceil(P / slice_paths)`` workgroups, cut as
        ``price_sliced_device`` cuts it: for one contract, or a few dozen, at a path count where one workgroup per
        contract leaves the chip idle.  Device tensors in and out, the current stream, no host sync.  With one slice
        the values are ``greeks_batch_device``'s bits; with more, the f64 sums are added slice by slice and the last
        bits may differ (the price columns stay ``price_sliced_device``'s bit for bit)."""
        res = self._greeks_sliced_block(contracts, slice_paths)
        if isinstance(res, Failure):
            return res
        return Success(self.BatchGreeks(**dict(zip(self.BatchGreeks.model_fields, res.value.unbind(dim=1)))))

    def greeks_sliced(self, inputs: "Sequence[BlackScholes.Inputs]", slice_paths: int | None = None
                      ) -> Result["list[BlackScholes.HostGreeks]", NormalsError]:
        """``greeks_batch`` through the sliced call: one device-to-host copy."""
        if self._cfg.path_scheme is not PathScheme.LOG_EULER:
            raise ValueError(f"greeks_sliced needs PathScheme.LOG_EULER, got {self._cfg.path_scheme.name}: the pathwise "
                             "Greeks are functions of the log-Euler terminal value")
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if len(inputs) == 0:
            return Success([])
        rows = [[float(getattr(c, f)) for f in FIELDS] for c in inputs]
        res = self._greeks_sliced_block(torch.tensor(rows, dtype=torch.float64, device=self._device()), slice_paths)
        if isinstance(res, Failure):
            return res
        names = list(self.BatchGreeks.model_fields)
        return Success([self.HostGreeks(**dict(zip(names, row))) for row in res.value.cpu().tolist()])

    # ------------------------------------------------------------------ batched Greeks of the path payoffs
    def _greeks_paths_block(self, contracts: torch.Tensor) -> Result[torch.Tensor, NormalsError]:
        """One ``smc_gbm_greeks_paths`` launch on the current stream (no sync): the ``[B, 40]`` f64 block of
        contracts ``[B, 6]`` f64 on the device; contract b takes ordinal ``ordinal + b``."""
        if self._cfg.path_scheme is not PathScheme.LOG_EULER:
            raise ValueError(f"greeks_paths_batch needs PathScheme.LOG_EULER, got {self._cfg.path_scheme.name}: the "
                             "pathwise Greeks are functions of the log-Euler row values")
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if contracts.ndim != 2 or contracts.shape[1] != len(FIELDS) or contracts.dtype != torch.float64:
            raise ValueError(f"contracts must be a [B, {len(FIELDS)}] float64 tensor, got "
                             f"{tuple(contracts.shape)} {contracts.dtype}")
        _lib.require_device()
        if not contracts.is_cuda:
            raise ValueError("contracts must be a device tensor")
        sp = self._sp
        contracts = contracts.contiguous()
        B = int(contracts.shape[0])
        block = torch.empty((B, _lib.PATH_GREEKS_COLS), dtype=torch.float64, device=contracts.device)
        if self.price_batch_math not in ("portable", "hw"):
            raise ValueError(f"price_batch_math must be 'portable' or 'hw', got {self.price_batch_math!r}")
        scheme = scheme_code(self._cfg.path_scheme) | (_lib.MATH_HW if self.price_batch_math == "hw" else 0)
        if B:
            _lib.check(_lib.lib().smc_gbm_greeks_paths(
                _lib.ptr(contracts), B, sp.timesteps, sp.total_paths(), sp.mc_seed, None, self._served,
                scheme, normalization_code(self._cfg.normalization), dtype_code(sp.dtype),
                _lib.ptr(block), _lib.stream_handle()))
            self._served += B
        return Success(block)

    def greeks_paths_batch_device(self, contracts: torch.Tensor
                                  ) -> Result["BlackScholes.PathBatchGreeks", NormalsError]:
        """Pathwise Greeks of the Asian and lookback put and call of B contracts (``[B, 6]`` f64 device tensor,
        columns X0 K T r d v) in one launch of the fused kernel, with no path matrix in memory and no host sync:
        the derivatives of the estimator ``price_paths_batch_device`` computes (without barriers), on the same
        paths, with their standard errors.  LOG_EULER engines only.  Consumes the normal streams of B ``price``
        calls."""
        res = self._greeks_paths_block(contracts)
        if isinstance(res, Failure):
            return res
        return Success(self.PathBatchGreeks(**dict(zip(self.PathBatchGreeks.model_fields, res.value.unbind(dim=1)))))

    def greeks_paths_batch(self, inputs: "Sequence[BlackScholes.Inputs]"
                           ) -> Result["list[BlackScholes.HostPathGreeks]", NormalsError]:
        """``greeks_paths_batch_device`` from host values: one launch and one device-to-host copy."""
        if self._cfg.path_scheme is not PathScheme.LOG_EULER:
            raise ValueError(f"greeks_paths_batch needs PathScheme.LOG_EULER, got {self._cfg.path_scheme.name}: the "
                             "pathwise Greeks are functions of the log-Euler row values")
        if self._normals_error is not None:
            return Failure(NormalsUnavailable(error=self._normals_error))
        if len(inputs) == 0:
            return Success([])
        rows = [[float(getattr(c, f)) for f in FIELDS] for c in inputs]
        res = self._greeks_paths_block(torch.tensor(rows, dtype=torch.float64, device=self._device()))
        if isinstance(res, Failure):
            return res
        names = list(self.PathBatchGreeks.model_fields)
        return Success([self.HostPathGreeks(**dict(zip(names, row))) for row in res.value.cpu().tolist()])


def intrinsic_values(contract: "BlackScholes.Inputs") -> tuple[float, float, float]:
    """(discount, forward, strike) used by ``predict_price`` (gbm_trainer.py:1746-1749)."""
    return exp(-contract.r * contract.T), contract.X0 * exp((contract.r - contract.d) * contract.T), contract.K


__all__ = ("BlackScholes", "BlackScholesConfig", "SimulationParams", "ThreadsPerBlock",
           "build_black_scholes_config", "build_simulation_params", "validate_simulation_params_memory")
