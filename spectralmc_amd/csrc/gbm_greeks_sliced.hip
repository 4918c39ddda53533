// Sliced batched Greeks (smc_gbm_greeks_sliced): one contract's [26] Greeks block across W workgroups.
//
// smc_gbm_price_sliced's geometry, streams and slice rule (gbm.hip, price_slice_kernel) carried over to
// greeks_kernel's block: a contract is cut into W = ceil(P / slice_paths) slices (slice_paths a multiple of
// kChunk, the last slice ends at P), one workgroup per (contract, slice): workgroup blockIdx.x = b W + w.  Inside
// its slice a workgroup is greeks_kernel over the slice's chunks (restated, not shared: greeks_kernel's registers
// stay as they are): the streams PathStream(seed, ordinal, p0 / 4, T) with the contract-global p0, the lane's 4
// raw terminal values summed in Real first, per lane over the slice's chunks in ascending order, wave butterfly
// xor 32..1, waves 0..7; lanes wholly past the slice end neither draw nor contribute.  Nothing survives a launch
// but the workspace, so there is no parked mode: NORMALIZE replays the slice's streams once the contract's two
// totals (sum x, sum f64(x L)) are known.
//
// The device code (EngineArgs, Stepper, lane_rows_s, Payoff, GreekConsts, greeks_add, ...) is gbm.hip's, compiled
// here device-only: its kernels are templates, so this translation unit holds none of them, and its host part and
// exported entry points stay in gbm.hip's own object.

#define SMC_GBM_DEVICE_ONLY
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "gbm.hip"
#pragma clang diagnostic pop

#pragma clang fp contract(off)

namespace smc {
namespace {

//   kGreekSliceRaw  RAW: sum x and the 20 sums of greeks_add at scale 1, one pass;
//   kGreekSliceSum  NORMALIZE pass 1: sum x and sum f64(x L) only;
//   kGreekSlicePay  NORMALIZE pass 2: the 20 sums with Payoff and GreekConsts from the contract's two totals.
// Workspace (doubles): partials [B][W][kGreekSliceSums] (greeks_add's 20 sums, then sum x, then sum x L), then
// totals [B][2] (sum x, sum x L).  Every slot read was written earlier in the same call (stream order): no zeroing,
// no atomics, no counters.  Under RAW the sum x L slot is neither written nor read.
enum GreekSlicePass : int { kGreekSliceRaw = 0, kGreekSliceSum = 1, kGreekSlicePay = 2 };
constexpr int kGreekSliceSums = kGreekSums + 2;
constexpr int kGreekSliceX = kGreekSums;       // partial kGreekSums: sum x
constexpr int kGreekSliceXL = kGreekSums + 1;  // partial kGreekSums + 1: sum f64(x L)
constexpr int kGreekFinishLanes = 32;          // threads per contract in greeks_finish_kernel (kGreekSliceSums add)

template <typename Real, bool HW, int PASS>
__global__ __launch_bounds__(kThreads) void greeks_slice_kernel(EngineArgs a, int64_t slice_paths, int32_t W,
                                                                double* __restrict__ ws) {
  extern __shared__ double lds[];  // price_reduce's [kWaves][2] scratch, then [kWaves][kGreekSums] over it
  if constexpr (sizeof(Real) == 8) math::f64_tables_load();
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / static_cast<uint32_t>(W);
  const int64_t w = blockIdx.x % static_cast<uint32_t>(W);
  const int T = a.T;
  const int64_t begin = w * slice_paths;  // < P: W = ceil(P / slice_paths)
  const int64_t end = a.P - begin > slice_paths ? begin + slice_paths : a.P;
  const double* const row = a.contracts + b * 6;
  const Contract c = load_contract(row);
  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);
  const Stepper<Real, true, HW> step(c, T);
  const Real x0 = static_cast<Real>(c.X0);
  double* slot = ws + (b * W + w) * kGreekSliceSums;

  auto valid_paths = [&](int64_t chunk) {  // how many of the lane's 4 values of this chunk are paths (< end)
    const int64_t p0 = chunk + kPathsPerLane * static_cast<int64_t>(tid);
    return static_cast<int>(p0 >= end ? 0 : (end - p0 >= kPathsPerLane ? kPathsPerLane : end - p0));
  };
  // the lane's 4 terminal values of one chunk (nvalid > 0)
  auto simulate = [&](int64_t chunk, Real (&xt)[kPathsPerLane]) {
    const int64_t p0 = chunk + kPathsPerLane * static_cast<int64_t>(tid);
    PathStream s(a.seed, ordinal, static_cast<uint64_t>(p0 / kPathsPerLane), T);
    double unused = 0.0;
    lane_rows_s<Real, true, HW, false, false>(s, step, x0, chunk, nullptr, T, 0, unused, xt, tid);
  };

  if constexpr (PASS == kGreekSliceSum) {
    double sum[2] = {0.0, 0.0};  // x, x L
    for (int64_t chunk = begin; chunk < end; chunk += kChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        Real xt[kPathsPerLane];
        simulate(chunk, xt);
        Real part = 0;
#pragma unroll
        for (int j = 0; j < kPathsPerLane; ++j) part += j < nvalid ? xt[j] : Real(0);
        sum[0] += static_cast<double>(part);
#pragma unroll
        for (int j = 0; j < kPathsPerLane; ++j)
          if (j < nvalid) sum[1] += static_cast<double>(xt[j] * greeks_log<Real, HW>(xt[j], x0));
      }
    }
    price_reduce(sum, lds);
    if (tid == 0) {
      slot[kGreekSliceX] = sum[0];
      slot[kGreekSliceXL] = sum[1];
    }
  } else {
    double v[kGreekSums];
#pragma unroll
    for (int i = 0; i < kGreekSums; ++i) v[i] = 0.0;
    double sum[1] = {0.0};
    // the contract row is read again: its six doubles are not held across the path loop
    const Contract cr = load_contract(row);
    const double* const tot = ws + a.B * W * kGreekSliceSums + b * 2;
    const double sumx = PASS == kGreekSlicePay ? tot[0] : 1.0;  // RAW: a.normalize == 0, scale 1
    const double sumxl = PASS == kGreekSlicePay ? tot[1] : 0.0;
    const Payoff<Real> pay(a, PayoffPre<Real>(cr), sumx);
    const GreekConsts<Real> g(cr, pay, PASS == kGreekSlicePay, sumx, sumxl);
    for (int64_t chunk = begin; chunk < end; chunk += kChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        Real xt[kPathsPerLane];
        simulate(chunk, xt);
        if constexpr (PASS == kGreekSliceRaw) {
          Real part = 0;
#pragma unroll
          for (int j = 0; j < kPathsPerLane; ++j) part += j < nvalid ? xt[j] : Real(0);
          sum[0] += static_cast<double>(part);
        }
#pragma unroll
        for (int j = 0; j < kPathsPerLane; ++j)
          if (j < nvalid) greeks_add<Real, HW>(pay, g, xt[j], v);
      }
    }
    if constexpr (PASS == kGreekSliceRaw) {
      price_reduce(sum, lds);
      if (tid == 0) slot[kGreekSliceX] = sum[0];
    }
    // greeks_kernel's final reduction: wave butterfly, then sum i totalled over waves 0..7 by thread i alone
    {
      const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
      for (int i = 0; i < kGreekSums; ++i) {
        const double s = wave_sum(v[i]);
        if (lane == 0) lds[wave * kGreekSums + i] = s;
      }
    }
    __syncthreads();
    if (tid < kGreekSums) {
      double t = 0.0;
      for (int k = 0; k < kWaves; ++k) t += lds[k * kGreekSums + tid];
      slot[tid] = t;
    }
  }
}

// Thread (b, k), k < kGreekSliceSums, adds partial k of contract b over the slices in order (slice 0's value, + slice
// 1, ...), so no thread holds more than one total.  totals_only: threads (b, kGreekSliceX) and (b, kGreekSliceXL)
// leave the two totals in the workspace (between the two NORMALIZE passes); else the 26 columns in greeks_kernel's
// closing arithmetic: thread (b, i), i < kGreekTerms, closes term i with the total of its squares from thread
// (b, kGreekTerms + i).
__global__ __launch_bounds__(kFinishThreads) void greeks_finish_kernel(EngineArgs a, int32_t W, int32_t totals_only,
                                                                       double* __restrict__ ws,
                                                                       double* __restrict__ greeks) {
  const int64_t b = static_cast<int64_t>(blockIdx.x) * (kFinishThreads / kGreekFinishLanes) +
                    threadIdx.x / kGreekFinishLanes;
  const int k = threadIdx.x % kGreekFinishLanes;
  const bool live = b < a.B;
  // which partials this call adds: the two pass-1 sums, or all that the slice passes wrote (RAW: no sum x L)
  const bool adds = totals_only ? (k == kGreekSliceX || k == kGreekSliceXL)
                                : (k < kGreekSliceSums && (a.normalize || k != kGreekSliceXL));
  double tot = 0.0;
  if (live && adds) {
    const double* part = ws + b * W * kGreekSliceSums + k;
    tot = part[0];
    // the adds stay in slice order; the loads of kFinishBatch slices are issued together, so the walk waits on
    // memory once per batch and not once per slice
    int32_t w = 1;
    for (; w + kFinishBatch <= W; w += kFinishBatch) {
      double t[kFinishBatch];
#pragma unroll
      for (int i = 0; i < kFinishBatch; ++i) t[i] = part[static_cast<int64_t>(w + i) * kGreekSliceSums];
#pragma unroll
      for (int i = 0; i < kFinishBatch; ++i) tot += t[i];
    }
    for (; w < W; ++w) tot += part[static_cast<int64_t>(w) * kGreekSliceSums];
  }
  if (totals_only) {
    if (live && adds) ws[a.B * W * kGreekSliceSums + b * 2 + (k - kGreekSliceX)] = tot;
    return;
  }
  // the total of term k's squares, from the contract's own 32-lane group (every lane takes part)
  const double sq = __shfl(tot, (threadIdx.x & 63) + (k < kGreekTerms ? kGreekTerms : 0), 64);
  if (!live) return;
  double* out = greeks + b * SMC_GREEKS_COLS;
  if (k < kGreekTerms) {  // term k: its mean and standard error
    const double n = static_cast<double>(a.P);
    const double m = tot / n;
    double se = 0.0;
    if (a.P > 1) {
      const double var = sq - n * m * m;
      se = sqrt((var > 0.0 ? var : 0.0) / (n - 1.0) / n);
    }
    if (k < 8) {
      out[k] = m;
      out[10 + k] = se;
    } else {  // the prices: columns 20, 21 and 22, 23
      out[12 + k] = m;
      out[14 + k] = se;
    }
    if (k == 2 || k == 3) {
      // gamma from the lognormal identity vega = v T X0^2 gamma (exact for the log-Euler terminal law)
      const Contract cr = load_contract(a.contracts + b * 6);
      const double vt = cr.v * cr.T;
      const double den = vt * cr.X0 * cr.X0;
      out[6 + k] = vt == 0.0 ? 0.0 : m / den;
      out[16 + k] = vt == 0.0 ? 0.0 : se / den;
    }
  } else if (k == kGreekSliceX) {
    out[24] = tot;
  } else if (k == kGreekSliceXL) {
    out[25] = a.normalize ? tot : 0.0;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
// Slices per contract: smc_gbm_price_sliced's rule (gbm.hip, price_slice_count); -1: not a (P, slice_paths) it takes
int64_t greeks_slice_count(int64_t P, int64_t slice_paths) {
  if (P <= 0 || P >= (1LL << 40) || slice_paths <= 0 || slice_paths % kChunk != 0) return -1;
  const int64_t W = (P + slice_paths - 1) / slice_paths;
  return W > 65535 ? -1 : W;
}

bool greeks_sliced_scheme_ok(int32_t scheme) {  // a base scheme and no flag but SMC_MATH_HW / SMC_MATH_REF
  const int32_t base = scheme & 0xff, flags = scheme & ~0xff;
  return (base == SMC_SCHEME_LOG_EULER || base == SMC_SCHEME_SIMPLE_EULER) &&
         (flags & ~(SMC_MATH_HW | SMC_MATH_REF)) == 0;
}

// The two (RAW) or four (NORMALIZE) launches of the sliced Greeks call, in stream order
template <typename Real, bool HW>
int32_t launch_greeks_sliced_k(const EngineArgs& a, int64_t slice_paths, int32_t W, double* ws, double* greeks,
                               hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(a.B * W)), block(kThreads);
  constexpr int kPerBlock = kFinishThreads / kGreekFinishLanes;
  const dim3 fgrid(static_cast<unsigned>((a.B + kPerBlock - 1) / kPerBlock)), fblock(kFinishThreads);
  const uint32_t lds = static_cast<uint32_t>(kGreekScratch);
  if (!a.normalize) {
    launch(greeks_slice_kernel<Real, HW, kGreekSliceRaw>, grid, block, lds, stream, a, slice_paths, W, ws);
    if (int32_t st = check_launch("greeks_slice_kernel")) return st;
  } else {
    launch(greeks_slice_kernel<Real, HW, kGreekSliceSum>, grid, block, lds, stream, a, slice_paths, W, ws);
    if (int32_t st = check_launch("greeks_slice_kernel")) return st;
    launch(greeks_finish_kernel, fgrid, fblock, 0, stream, a, W, 1, ws, greeks);
    if (int32_t st = check_launch("greeks_finish_kernel")) return st;
    launch(greeks_slice_kernel<Real, HW, kGreekSlicePay>, grid, block, lds, stream, a, slice_paths, W, ws);
    if (int32_t st = check_launch("greeks_slice_kernel")) return st;
  }
  launch(greeks_finish_kernel, fgrid, fblock, 0, stream, a, W, 0, ws, greeks);
  return check_launch("greeks_finish_kernel");
}

template <typename Real>
int32_t launch_greeks_sliced(const EngineArgs& a, int64_t slice_paths, int32_t W, double* ws, double* greeks,
                             hipStream_t stream) {
  if constexpr (sizeof(Real) == 4) {
    if (a.scheme & SMC_MATH_HW) return launch_greeks_sliced_k<Real, true>(a, slice_paths, W, ws, greeks, stream);
  }
  return launch_greeks_sliced_k<Real, false>(a, slice_paths, W, ws, greeks, stream);
}

}  // namespace
}  // namespace smc

using namespace smc;

extern "C" {
#pragma GCC visibility push(default)

int32_t smc_gbm_greeks_sliced(const double* contracts_dev, int64_t n_contracts, int32_t timesteps, int64_t n_paths,
                              int64_t slice_paths, uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0,
                              int32_t scheme, int32_t normalization, int32_t dtype, double* greeks_dev,
                              void* workspace_dev, int64_t workspace_bytes, void* stream) {
  constexpr int32_t kNoMode = SMC_PRICE_REPLAY | SMC_TRAIN_DYNAMIC;
  // 1. smc_gbm_greeks' checks
  if (!contracts_dev) return fail(SMC_ERR_INVALID_ARGUMENT, "smc_gbm_greeks_sliced: contracts is NULL");
  if (n_contracts < 0 || timesteps <= 0 || n_paths <= 0)
    return fail(SMC_ERR_INVALID_SHAPE, "smc_gbm_greeks_sliced: need B >= 0, T > 0, P > 0");
  if (n_contracts > 0x7fffffffLL)
    return fail(SMC_ERR_INVALID_SHAPE, "smc_gbm_greeks_sliced: more than 2^31-1 contracts in one call");
  if (n_paths >= (1LL << 40)) return fail(SMC_ERR_INVALID_SHAPE, "smc_gbm_greeks_sliced: path count too large");
  if (dtype != SMC_DTYPE_F32 && dtype != SMC_DTYPE_F64)
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_gbm_greeks_sliced: bad dtype");
  if (!greeks_dev) return fail(SMC_ERR_INVALID_ARGUMENT, "smc_gbm_greeks_sliced: greeks_dev is NULL");
  if (!greeks_sliced_scheme_ok(scheme & ~kNoMode))
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_gbm_greeks_sliced: bad scheme");
  if (scheme & SMC_MATH_REF)
    return fail(SMC_ERR_INVALID_ARGUMENT,
                "smc_gbm_greeks_sliced: SMC_MATH_REF is for smc_train_targets / smc_train_step");
  if ((scheme & SMC_MATH_HW) && dtype == SMC_DTYPE_F64)
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_gbm_greeks_sliced: SMC_MATH_HW is f32 only");
  if (normalization != SMC_NORM_RAW && normalization != SMC_NORM_NORMALIZE)
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_gbm_greeks_sliced: bad normalization");
  if ((scheme & 0xff) != SMC_SCHEME_LOG_EULER)
    return fail(SMC_ERR_INVALID_ARGUMENT,
                "smc_gbm_greeks_sliced: SMC_SCHEME_SIMPLE_EULER is not supported (the reflected step is not a "
                "function of the terminal value); use SMC_SCHEME_LOG_EULER");
  // 2. there is no mode to force
  if (scheme & kNoMode)
    return fail(SMC_ERR_INVALID_ARGUMENT,
                "smc_gbm_greeks_sliced: SMC_PRICE_REPLAY / SMC_TRAIN_DYNAMIC do not apply (there is no mode to force)");
  // 3. the slice length, the grid and the workspace: smc_gbm_price_sliced's checks and codes
  if (slice_paths <= 0 || slice_paths % kChunk != 0)
    return fail(SMC_ERR_INVALID_SHAPE, "smc_gbm_greeks_sliced: slice_paths must be a positive multiple of 2048");
  const int64_t W = greeks_slice_count(n_paths, slice_paths);
  if (W < 0 || n_contracts * W >= (1LL << 31))
    return fail(SMC_ERR_INVALID_SHAPE,
                "smc_gbm_greeks_sliced: more than 65,535 slices per contract, or 2^31 or more workgroups");
  if (!workspace_dev) return fail(SMC_ERR_INVALID_ARGUMENT, "smc_gbm_greeks_sliced: workspace_dev is NULL");
  if (workspace_bytes < smc_gbm_greeks_sliced_workspace_bytes(n_contracts, n_paths, slice_paths))
    return fail(SMC_ERR_INVALID_ARGUMENT,
                "smc_gbm_greeks_sliced: workspace_bytes below smc_gbm_greeks_sliced_workspace_bytes");
  if (n_contracts == 0) return SMC_OK;
  EngineArgs a{};
  a.contracts = contracts_dev;
  a.B = n_contracts;
  a.T = timesteps;
  a.P = n_paths;
  a.seed = mc_seed;
  a.ordinal_dev = ordinal_dev;
  a.ordinal0 = ordinal0;
  a.scheme = scheme;
  a.normalize = normalization != SMC_NORM_RAW;
  double* ws = static_cast<double*>(workspace_dev);
  return dtype == SMC_DTYPE_F32
             ? launch_greeks_sliced<float>(a, slice_paths, static_cast<int32_t>(W), ws, greeks_dev, as_stream(stream))
             : launch_greeks_sliced<double>(a, slice_paths, static_cast<int32_t>(W), ws, greeks_dev, as_stream(stream));
}

int64_t smc_gbm_greeks_sliced_workspace_bytes(int64_t n_contracts, int64_t n_paths, int64_t slice_paths) {
  const int64_t W = greeks_slice_count(n_paths, slice_paths);
  if (n_contracts < 0 || n_contracts > 0x7fffffffLL || W < 0 || n_contracts * W >= (1LL << 31)) return -1;
  return static_cast<int64_t>(sizeof(double)) * n_contracts * (kGreekSliceSums * W + 2);
}

const char* smc_gbm_greeks_sliced_kernel(int32_t timesteps, int64_t n_paths, int64_t slice_paths, int32_t scheme,
                                         int32_t normalization, int32_t dtype) {
  if (timesteps <= 0 || greeks_slice_count(n_paths, slice_paths) < 0 || !greeks_sliced_scheme_ok(scheme) ||
      (scheme & 0xff) != SMC_SCHEME_LOG_EULER || (scheme & SMC_MATH_REF) ||
      (dtype != SMC_DTYPE_F32 && dtype != SMC_DTYPE_F64) || ((scheme & SMC_MATH_HW) && dtype == SMC_DTYPE_F64))
    return "unsupported";
  if (normalization == SMC_NORM_RAW) return "greeks_slice_kernel(raw)";
  if (normalization == SMC_NORM_NORMALIZE) return "greeks_slice_kernel(replay)";
  return "unsupported";
}

#pragma GCC visibility pop
}  // extern "C"
