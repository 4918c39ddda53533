// Correlated multi-asset GBM engine for gfx950 (BASELINE.json configs[4]: "multi-asset
// correlated GBM, 4 assets, Cholesky in LDS"): A assets per contract, equicorrelated
// Brownian drivers, equal-weight basket put, CF training targets.
//
// This is an extension of the reference's single-asset engine; each asset follows the
// reference dynamics (src/spectralmc/gbm.py:224-257, log-Euler) and forward normalisation
// (gbm.py:428-440); the payoff is the builder-defined basket put
//   df_T * max(K - (1/A) sum_i x_i,T * F_i / mean_p(x_i,T), 0)
// and the target is mean_m FFT_N(put.reshape(M, N)) as gbm_trainer.py:806-817.
//
// Contract row (f64, width 3A + 4): K, T, r, rho, X0[0..A), d[0..A), v[0..A).
// Correlation matrix C = (1 - rho) I + rho 11^T, factored C = L L^T once per workgroup in LDS.
//
// Layout: paths [B][A][T][pitch] f32 (STORE_ALL) or [B][A][pitch] (terminal rows only), so each
// asset's block is a single-asset [T][P] matrix.  basket_kernel: one 512-thread workgroup per
// contract; each lane owns 4 consecutive paths of a 2048-path chunk for all A assets and stores
// one dwordx4 per (asset, row).  basket_resident_kernel (the C5 kernel, below): W = P / 4096
// co-resident 1024-thread workgroups per contract keep the terminal rows on chip.
// basket_price_kernel (smc_basket_price): basket_kernel's geometry with no row stored; the equal-weight
// basket, best-of and worst-of prices of a contract leave as 18 doubles.
//
// Per lane, per step t, per path j = 0..3: ceil(A/2) Box-Muller pairs from the lane's
// PathStream (smc_rng.h; the same (seed, contract ordinal, group) keying as the single-asset
// engine) -> z[0..A) (an odd A discards the last pair's second normal);
// y_i = a_i + sum_{k<=i} (b_i L_ik) z_k (f32 fma chain in k order, b_i L_ik rounded once from f64);
// x_i *= 2^y_i.  oracle/gbm_oracle.c (oracle_basket_kernel) restates this bit for bit
// in portable math.

#include <cmath>
#include <type_traits>
#include <utility>

#pragma clang fp contract(off)

#include "smc_internal.h"
#include "smc_math.h"
#include "smc_rng.h"
#include "smc_device.h"

namespace smc {
namespace {

constexpr int kBThreads = 512;
constexpr int kBWaves = kBThreads / 64;
constexpr int kBPaths = 4;                      // paths per lane
constexpr int kBChunk = kBThreads * kBPaths;    // paths per workgroup pass
constexpr int kMaxAssets = 8;
constexpr double kBLog2e = 1.4426950408889634;

struct BasketArgs {
  const double* contracts;  // [B][3A + 4] of this launch
  int64_t B;
  int32_t T;
  int64_t P;
  int32_t N, M;
  uint64_t seed;
  const int64_t* ordinal_dev;
  int64_t ordinal0;
  int32_t normalize;
  int32_t store_all;
  float* paths;
  int64_t pitch;            // elements between consecutive rows
  double* terminal_sum;     // [B][A] or NULL
  float2* targets;          // [B][N]
};

__device__ __forceinline__ double bwave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// Cholesky-Banachiewicz of the equicorrelation matrix in LDS (f64, one thread; A <= 8).
__device__ void cholesky_equicorr(int A, double rho, double* L) {
  for (int i = 0; i < A; ++i)
    for (int k = 0; k <= i; ++k) {
      double s = i == k ? 1.0 : rho;
      for (int m = 0; m < k; ++m) s = s - L[i * kMaxAssets + m] * L[k * kMaxAssets + m];
      L[i * kMaxAssets + k] = i == k ? sqrt(s > 0.0 ? s : 0.0) : s / L[k * kMaxAssets + k];
    }
}

// Payoff + M-mean + DFT of contract b from its stored terminal rows and their sums tot[A] (in
// LDS): the CF phase of basket_kernel, and all of basket_cf_kernel.
template <int A>
__device__ void basket_cf(const BasketArgs& a, int64_t b, const double* tot, double* part, double* avg,
                          const double* cs, const double* sn) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x;
  const int N = a.N, M = a.M;
  const int64_t P = a.P;
  const double* c = a.contracts + b * (3 * A + 4);
  const double K = c[0], Tm = c[1], r = c[2];
  const int64_t rows = a.store_all ? a.T : 1;
  const float* cbase = a.paths + b * A * rows * a.pitch;
  // payoff: per-asset forward scale, equal-weight basket, discounted put (f32, asset order)
  const float Tf = static_cast<float>(Tm);
  const float df = math::exp_any(static_cast<float>(-r) * Tf);
  const float Kf = static_cast<float>(K);
  const float wA = static_cast<float>(1.0 / A);
  float sc[A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const float F = static_cast<float>(c[4 + i]) * math::exp_any(static_cast<float>(r - c[4 + A + i]) * Tf);
    sc[i] = a.normalize ? F / static_cast<float>(tot[i] / static_cast<double>(P)) : 1.0f;
  }
  __amdgpu_buffer_rsrc_t rs[A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const float* trow = cbase + (i * rows + (rows - 1)) * a.pitch;
    rs[i] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(trow), static_cast<short>(0), 0x7fffffff,
                                              0x00020000);
  }
  // thread item (q, g): columns 4q..4q+3, batches m = g, g + G, ... (oracle_basket_kernel order)
  const int cols = N / 4;
  const int G = cols <= kBThreads ? kBThreads / cols : 1;
  const int items = cols * G;
  constexpr int kB = A <= 2 ? 8 : (A <= 4 ? 4 : 2);  // batches in flight per thread
  for (int item = tid; item < items; item += kBThreads) {
    const int q = item % cols, g = item / cols;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m0 = g; m0 < M; m0 += G * kB) {
      v4f v[kB][A];
#pragma unroll
      for (int u = 0; u < kB; ++u) {
        const int m = m0 + u * G < M ? m0 + u * G : M - 1;
#pragma unroll
        for (int i = 0; i < A; ++i)
          v[u][i] = __builtin_amdgcn_raw_buffer_load_b128(rs[i], (m * N + 4 * q) * 4, 0, 16 /* sc1 */);
      }
#pragma unroll
      for (int u = 0; u < kB; ++u) {
        if (m0 + u * G < M) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float bs = 0.0f;
#pragma unroll
            for (int i = 0; i < A; ++i) bs = bs + v[u][i][e] * sc[i];
            const float diff = Kf - bs * wA;
            sum[e] += static_cast<double>(df * (diff > 0.0f ? diff : 0.0f));
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) part[g * N + 4 * q + e] = sum[e];
  }
  __syncthreads();
  for (int n = tid; n < N; n += kBThreads) {
    double t2 = 0.0;
    for (int g = 0; g < G; ++g) t2 += part[g * N + n];
    avg[n] = t2 / static_cast<double>(M);
  }
  __syncthreads();
  float2* out = a.targets + b * N;
  for (int k = tid; k <= N / 2; k += kBThreads) {
    double re = 0.0, im = 0.0;
    int idx = 0;
    for (int n = 0; n < N; ++n) {
      re = fma(avg[n], cs[idx], re);
      im = fma(-avg[n], sn[idx], im);
      idx += k;
      if (idx >= N) idx -= N;
    }
    out[k] = make_float2(static_cast<float>(re), static_cast<float>(im));
    if (k != 0 && 2 * k != N) out[N - k] = make_float2(static_cast<float>(re), static_cast<float>(-im));
  }
}

template <int A, bool HW, int MODE>  // MODE 0: simulate + CF, 1: simulate only (terminal sums out)
__global__ __launch_bounds__(kBThreads) void basket_kernel(BasketArgs a) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T = a.T, N = a.N;
  const int64_t P = a.P;
  double* Ld = lds;                          // [8][8]
  double* wsum = Ld + kMaxAssets * kMaxAssets;  // [kBWaves][A]
  double* tot = wsum + kBWaves * A;          // [A]
  double* part = tot + A;                    // [max(4 kBThreads, N)]
  double* avg = part + (N > 4 * kBThreads ? N : 4 * kBThreads);  // [N]
  double* cs = avg + N;
  double* sn = cs + N;

  const double* c = a.contracts + b * (3 * A + 4);
  const double Tm = c[1], r = c[2], rho = c[3];
  if (tid == 0) cholesky_equicorr(A, rho, Ld);
  if (MODE == 0)
    for (int j = tid; j < N; j += kBThreads) math::twiddle(j, N, sn[j], cs[j]);
  __syncthreads();

  // per-asset log2-unit coefficients (Stepper of gbm.hip); HW normals come out / sqrt(2 ln 2)
  const double dt = Tm / static_cast<double>(T);
  const double sq = sqrt(dt);
  constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
  // y_i = a_i + sum_{k <= i} (b_i L_ik) z_k: the volatility coefficient is folded into the factor
  float ca[A], x0[A], Lb[A][A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double drift = r - d - 0.5 * v * v;
    ca[i] = static_cast<float>(drift * dt * kBLog2e);
    const double bi = v * sq * kBLog2e * zscale;
    x0[i] = static_cast<float>(c[4 + i]);
#pragma unroll
    for (int k = 0; k < A; ++k) Lb[i][k] = k <= i ? static_cast<float>(bi * Ld[i * kMaxAssets + k]) : 0.0f;
  }

  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);
  const int64_t pitch = a.pitch;
  const int64_t rows = a.store_all ? T : 1;
  float* cbase = a.paths + b * A * rows * pitch;
  const uint32_t lane_off = static_cast<uint32_t>(kBPaths * sizeof(float)) * tid;
  double acc[A];
#pragma unroll
  for (int i = 0; i < A; ++i) acc[i] = 0.0;

  for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
    PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
    float x[A][kBPaths];
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
      for (int j = 0; j < kBPaths; ++j) x[i][j] = x0[i];
    for (int t = 0; t < T; ++t) {
      // path pairs (j, j + 1): draws in path order, then the correlation and the step as packed
      // f32 ops (v_pk_fma_f32 / v_pk_mul_f32; same IEEE results as the scalar ops)
#pragma unroll
      for (int j = 0; j < kBPaths; j += 2) {
        float z0[A + 1], z1[A + 1];
#pragma unroll
        for (int k = 0; k < A; k += 2) s.template normal_pair<HW>(z0[k], z0[k + 1]);
#pragma unroll
        for (int k = 0; k < A; k += 2) s.template normal_pair<HW>(z1[k], z1[k + 1]);
#pragma unroll
        for (int i = 0; i < A; ++i) {
          f2 y = {ca[i], ca[i]};
#pragma unroll
          for (int k = 0; k <= i; ++k) y = __builtin_elementwise_fma(f2{Lb[i][k], Lb[i][k]}, f2{z0[k], z1[k]}, y);
          f2 e;
          if constexpr (HW) e = f2{__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)};
          else e = f2{math::exp2_any(y.x), math::exp2_any(y.y)};
          const f2 xv = f2{x[i][j], x[i][j + 1]} * e;
          x[i][j] = xv.x;
          x[i][j + 1] = xv.y;
        }
      }
      if (a.store_all || t == T - 1) {
        const int64_t row = a.store_all ? t : 0;
#pragma unroll
        for (int i = 0; i < A; ++i) {
          const v4f v = {x[i][0], x[i][1], x[i][2], x[i][3]};
          char* rb = reinterpret_cast<char*>(cbase + (i * rows + row) * pitch + chunk);
          *reinterpret_cast<v4f*>(rb + lane_off) = v;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < A; ++i) {
      float p = 0.0f;
#pragma unroll
      for (int j = 0; j < kBPaths; ++j) p += x[i][j];
      acc[i] += static_cast<double>(p);
    }
  }

  // terminal sums: lane over chunks, wave butterfly, waves 0..7 (fixed order)
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double w = bwave_sum(acc[i]);
    if (lane == 0) wsum[wave * A + i] = w;
  }
  __syncthreads();
  if (tid < A) {
    double sum = 0.0;
    for (int w = 0; w < kBWaves; ++w) sum += wsum[w * A + tid];
    tot[tid] = sum;
    if (a.terminal_sum) a.terminal_sum[b * A + tid] = sum;
  }
  if constexpr (MODE == 1) return;  // basket_cf_kernel takes it from the stored rows and sums
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this workgroup's terminal-row stores
  __syncthreads();
  basket_cf<A>(a, b, tot, part, avg, cs, sn);
}

// One workgroup per contract: the CF phase from the stored terminal rows and terminal sums
// (a separate pass after basket_kernel<MODE 1>: bit-identical to the fused kernel).
template <int A>
__global__ __launch_bounds__(kBThreads) void basket_cf_kernel(BasketArgs a) {
  extern __shared__ double lds[];
  const int N = a.N;
  const int64_t b = blockIdx.x;
  double* tot = lds;                         // [A]
  double* part = tot + kMaxAssets;           // [max(4 kBThreads, N)]
  double* avg = part + (N > 4 * kBThreads ? N : 4 * kBThreads);  // [N]
  double* cs = avg + N;
  double* sn = cs + N;
  for (int j = threadIdx.x; j < N; j += kBThreads) math::twiddle(j, N, sn[j], cs[j]);
  if (threadIdx.x < A) tot[threadIdx.x] = a.terminal_sum[b * A + threadIdx.x];
  __syncthreads();
  basket_cf<A>(a, b, tot, part, avg, cs, sn);
}

// ---- batched basket pricing: basket_price_kernel (smc_basket_price) ------------------------------
// basket_kernel's geometry, streams and step (one 512-lane workgroup per contract, 4 consecutive paths
// of every 2048-path chunk per lane for all A assets, PathStream(seed, ordinal, chunk / 4 + tid), draws
// in path pairs, the packed f32 step), with no row stored: the A scaled terminal values of a path are
// seen in registers, xs_i = x_i s_i with basket_cf's scale s_i = F_i / f32(tot_i / P) (1 under RAW), and
// give the equal-weight basket bk = (((0 + xs_0) + xs_1) + ...) f32(1 / A), the best mx = max_i xs_i and
// the worst mn = min_i xs_i.  Six payoffs per path (put and call on each, df max(. , 0) in f32, cast to
// f64) and kBPriceSums f64 sums per contract: the payoffs, their squares, bk, mx, mn and the count of
// paths with bk < K.  Any P >= 1: a lane whose 4 paths lie wholly past P neither draws nor contributes,
// one with 1 to 3 paths draws for all 4 (the stream is per group of 4) and counts the valid ones.
// Terminal sums: the lane's valid values left to right in f32 from 0, then f64 per lane over its chunks,
// wave butterfly, waves 0..7 (basket_kernel's order, bit for bit where 2048 | P).  Payoff sums: per lane
// over its chunks and paths in order, wave butterfly, waves 0..7, sum i totalled by thread i.
//   kBPriceRaw     RAW normalisation: one pass, the payoffs taken as the paths finish;
//   kBPriceLds     NORMALIZE: each lane parks its terminal values in dynamic LDS ([A][P rounded up to 4]
//                  f32, one 16-B slot per lane, chunk and asset; a lane reads back only what it wrote)
//                  and takes the payoffs from there once the A sums are known;
//   kBPriceReplay  NORMALIZE, the parked block too large (or SMC_PRICE_REPLAY): pass 1 gives the sums,
//                  pass 2 re-creates the same streams: kBPriceLds' values and order, so the same bits.
// Contract values are not validated: an indefinite correlation matrix gives NaN, and rho = 1 is only
// meaningful for A <= 2 (from A = 3 on the factorisation divides 0 by 0).
enum BasketPriceMode : int { kBPriceRaw = 0, kBPriceLds = 1, kBPriceReplay = 2 };
constexpr int kBPriceSums = 16;  // 6 payoffs, their squares, bk, mx, mn, count(bk < K)
// scratch at the head of the dynamic LDS: payoff-sum partials [kBWaves][kBPriceSums], the Cholesky factor
// [8][8], terminal-sum partials [kBWaves][8] and totals [8] (f64; 2112 B, a multiple of 16)
constexpr int kBPriceHead = kBWaves * kBPriceSums + kMaxAssets * kMaxAssets + kBWaves * kMaxAssets + kMaxAssets;
constexpr size_t kBPriceScratch = kBPriceHead * sizeof(double);
// Largest dynamic LDS (scratch + parked block) of the lds mode: price_kernel's bound (gbm.hip)
#ifndef SMC_PRICE_PARK_BYTES
#define SMC_PRICE_PARK_BYTES (144 * 1024)
#endif
constexpr size_t kBPriceParkBytes = SMC_PRICE_PARK_BYTES;

// The lane's 4 paths of all A assets of one chunk from x0 through the T steps: basket_kernel's path loop
// without its row stores (the same draws and packed f32 ops in the same order).
// hook (basket_path_kernel): called as hook(x, t) after the step that makes row t, with the lane's 4 values of
// every asset; the default does nothing and leaves the callers' code as it was.
struct NoBasketRowHook {
  template <typename X>
  __device__ __forceinline__ void operator()(const X&, int) const {}
};

template <int A, bool HW, typename Hook = NoBasketRowHook>
__device__ __forceinline__ void basket_lane_paths(PathStream& s, const float (&ca)[A], const float (&x0)[A],
                                                  const float (&Lb)[A][A], int T, float (&x)[A][kBPaths],
                                                  Hook&& hook = Hook()) {
  typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int j = 0; j < kBPaths; ++j) x[i][j] = x0[i];
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int j = 0; j < kBPaths; j += 2) {
      float z0[A + 1], z1[A + 1];
#pragma unroll
      for (int k = 0; k < A; k += 2) s.template normal_pair<HW>(z0[k], z0[k + 1]);
#pragma unroll
      for (int k = 0; k < A; k += 2) s.template normal_pair<HW>(z1[k], z1[k + 1]);
#pragma unroll
      for (int i = 0; i < A; ++i) {
        f2 y = {ca[i], ca[i]};
#pragma unroll
        for (int k = 0; k <= i; ++k) y = __builtin_elementwise_fma(f2{Lb[i][k], Lb[i][k]}, f2{z0[k], z1[k]}, y);
        f2 e;
        if constexpr (HW) e = f2{__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)};
        else e = f2{math::exp2_any(y.x), math::exp2_any(y.y)};
        const f2 xv = f2{x[i][j], x[i][j + 1]} * e;
        x[i][j] = xv.x;
        x[i][j + 1] = xv.y;
      }
    }
    hook(x, t);
  }
}

template <int A, bool HW, int MODE>
__global__ __launch_bounds__(kBThreads) void basket_price_kernel(BasketArgs a, double* __restrict__ prices) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  extern __shared__ double lds[];  // kBPriceHead doubles of scratch, then (kBPriceLds) the parked block
  double* Ld = lds + kBWaves * kBPriceSums;     // [8][8]
  double* wsum = Ld + kMaxAssets * kMaxAssets;  // [kBWaves][A]
  double* tot = wsum + kBWaves * kMaxAssets;    // [A]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T = a.T;
  const int64_t P = a.P;
  const int64_t P4 = (P + 3) & ~int64_t{3};  // the parked block's row length
  v4f* park = reinterpret_cast<v4f*>(lds + kBPriceHead);

  const double* c = a.contracts + b * (3 * A + 4);
  const double Tm = c[1], r = c[2], rho = c[3];
  if (tid == 0) cholesky_equicorr(A, rho, Ld);
  __syncthreads();
  // per-asset log2-unit coefficients, as basket_kernel
  const double dt = Tm / static_cast<double>(T);
  const double sq = sqrt(dt);
  constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
  float ca[A], x0[A], Lb[A][A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double drift = r - d - 0.5 * v * v;
    ca[i] = static_cast<float>(drift * dt * kBLog2e);
    const double bi = v * sq * kBLog2e * zscale;
    x0[i] = static_cast<float>(c[4 + i]);
#pragma unroll
    for (int k = 0; k < A; ++k) Lb[i][k] = k <= i ? static_cast<float>(bi * Ld[i * kMaxAssets + k]) : 0.0f;
  }
  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);

  // payoff constants (basket_cf's arithmetic)
  const float Tf = static_cast<float>(Tm);
  const float df = math::exp_any(static_cast<float>(-r) * Tf);
  const float Kf = static_cast<float>(c[0]);
  const float wA = static_cast<float>(1.0 / A);
  auto forward = [&](int i) {
    return static_cast<float>(c[4 + i]) * math::exp_any(static_cast<float>(r - c[4 + A + i]) * Tf);
  };
  auto valid_paths = [&](int64_t chunk) {  // how many of the lane's 4 values of this chunk are paths (< P)
    const int64_t left = P - chunk - kBPaths * static_cast<int64_t>(tid);
    return static_cast<int>(left <= 0 ? 0 : (left >= kBPaths ? kBPaths : left));
  };
  auto simulate = [&](int64_t chunk, float(&x)[A][kBPaths]) {
    PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
    basket_lane_paths<A, HW>(s, ca, x0, Lb, T, x);
  };
  double v[kBPriceSums];
#pragma unroll
  for (int i = 0; i < kBPriceSums; ++i) v[i] = 0.0;
  auto payoffs = [&](const float(&x)[A][kBPaths], int nvalid, const float(&sc)[A]) {
    auto pay = [&](float diff) { return static_cast<double>(df * (diff > 0.0f ? diff : 0.0f)); };
#pragma unroll
    for (int j = 0; j < kBPaths; ++j) {
      if (j < nvalid) {
        float bs = 0.0f, mx = 0.0f, mn = 0.0f;
#pragma unroll
        for (int i = 0; i < A; ++i) {
          const float xs = x[i][j] * sc[i];
          bs = bs + xs;
          mx = i == 0 || xs > mx ? xs : mx;
          mn = i == 0 || xs < mn ? xs : mn;
        }
        const float bk = bs * wA;
        const double p[6] = {pay(Kf - bk), pay(bk - Kf), pay(Kf - mx), pay(mx - Kf), pay(Kf - mn), pay(mn - Kf)};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          v[i] += p[i];
          v[6 + i] += p[i] * p[i];
        }
        v[12] += static_cast<double>(bk);
        v[13] += static_cast<double>(mx);
        v[14] += static_cast<double>(mn);
        v[15] += bk < Kf ? 1.0 : 0.0;
      }
    }
  };

  // pass 1: the terminal sums (RAW: and the payoffs, scale 1; lds: and the parked values)
  float sc[A];
#pragma unroll
  for (int i = 0; i < A; ++i) sc[i] = 1.0f;
  double acc[A];
#pragma unroll
  for (int i = 0; i < A; ++i) acc[i] = 0.0;
  for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
    const int nvalid = valid_paths(chunk);
    if (nvalid > 0) {
      float x[A][kBPaths];
      simulate(chunk, x);
#pragma unroll
      for (int i = 0; i < A; ++i) {
        float p = 0.0f;
#pragma unroll
        for (int j = 0; j < kBPaths; ++j) p += j < nvalid ? x[i][j] : 0.0f;
        acc[i] += static_cast<double>(p);
      }
      if constexpr (MODE == kBPriceRaw) payoffs(x, nvalid, sc);
      if constexpr (MODE == kBPriceLds) {
        // slot (chunk + 4 tid) / 4 of row i: chunk + 4 tid < P, so the slot ends at or before P4
#pragma unroll
        for (int i = 0; i < A; ++i)
          park[(i * P4 + chunk) / kBPaths + tid] = v4f{x[i][0], x[i][1], x[i][2], x[i][3]};
      }
    }
  }
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double w = bwave_sum(acc[i]);
    if (lane == 0) wsum[wave * A + i] = w;
  }
  __syncthreads();
  if (tid < A) {
    double sum = 0.0;
    for (int w = 0; w < kBWaves; ++w) sum += wsum[w * A + tid];
    tot[tid] = sum;
    if (a.terminal_sum) a.terminal_sum[b * A + tid] = sum;
  }
  if constexpr (MODE != kBPriceRaw) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < A; ++i) sc[i] = forward(i) / static_cast<float>(tot[i] / static_cast<double>(P));
    // pass 2: the payoffs of the lane's own values, parked or simulated again
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float x[A][kBPaths];
        if constexpr (MODE == kBPriceLds) {
#pragma unroll
          for (int i = 0; i < A; ++i) {
            const v4f q = park[(i * P4 + chunk) / kBPaths + tid];
#pragma unroll
            for (int j = 0; j < kBPaths; ++j) x[i][j] = q[j];
          }
        } else {
          simulate(chunk, x);
        }
        payoffs(x, nvalid, sc);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kBPriceSums; ++i) {
    const double w = bwave_sum(v[i]);
    if (lane == 0) lds[wave * kBPriceSums + i] = w;
  }
  __syncthreads();
  auto total = [&](int i) {
    double t = 0.0;
    for (int w = 0; w < kBWaves; ++w) t += lds[w * kBPriceSums + i];
    return t;
  };
  const double n = static_cast<double>(P);
  double* out = prices + b * SMC_BASKET_PRICE_COLS;
  if (tid < 6) {  // a payoff's mean and standard error
    const double m = total(tid) / n;
    double se = 0.0;
    if (P > 1) {
      const double var = total(6 + tid) - n * m * m;
      se = sqrt((var > 0.0 ? var : 0.0) / (n - 1.0) / n);
    }
    out[tid] = m;
    out[6 + tid] = se;
  } else if (tid >= 12 && tid < kBPriceSums) {  // means of bk, mx, mn; the exercise share
    out[tid] = total(tid) / n;
  } else if (tid == kBPriceSums) {  // intrinsic basket put / call
    float fs = 0.0f;
#pragma unroll
    for (int i = 0; i < A; ++i) fs = fs + forward(i);
    const float ip = Kf - fs * wA, ic = fs * wA - Kf;
    out[16] = static_cast<double>(df * (ip > 0.0f ? ip : 0.0f));
    out[17] = static_cast<double>(df * (ic > 0.0f ? ic : 0.0f));
  }
}

// ---- weighted, general-correlation basket pricing: basket_general_kernel (smc_basket_price_general) ----
// basket_price_kernel's geometry, streams, chunk / validity handling, modes and sum orders (restated, not shared:
// basket_price_kernel's registers stay as they are; the path loop is basket_lane_paths), with two things the
// caller now supplies per contract.  The correlation matrix: its strict lower triangle, packed row by row
// ((1,0), (2,0), (2,1), (3,0), ...), goes through cholesky_equicorr's statements with rho replaced by C_ik; no
// matrix (corr NULL) means C_ik = rho, the same statements on the same values.  The weights: w_i = f32 of the
// caller's f64 (f32(1 / A) without a row), and the basket is bk = (((0 + w_0 xs_0) + w_1 xs_1) + ...), every
// operation rounded; mx and mn stay over the unweighted xs_i.  Weights may be negative (spreads) and are not
// normalised.  Stride 0 shares row 0 of either table with every contract.  Scratch: basket_price_kernel's
// kBPriceHead doubles (2112 B; the factor is built from global memory, the weights live in registers), so the
// lds -> replay switch falls at the same P as the price kernel's.  Nothing is validated: an indefinite matrix
// gives non-finite or meaningless rows.
struct BasketGeneralArgs {
  const double* weights;  // rows of A, or NULL
  int64_t weights_stride;
  const double* corr;     // rows of A (A - 1) / 2, or NULL
  int64_t corr_stride;
};
constexpr int kBGeneralHead = kBPriceHead;
constexpr size_t kBGeneralScratch = kBGeneralHead * sizeof(double);

// cholesky_equicorr with C_ik (k < i) from the packed triangle tri, or rho where tri is NULL.
__device__ void cholesky_general(int A, double rho, const double* tri, double* L) {
  for (int i = 0; i < A; ++i)
    for (int k = 0; k <= i; ++k) {
      double s = i == k ? 1.0 : (tri ? tri[i * (i - 1) / 2 + k] : rho);
      for (int m = 0; m < k; ++m) s = s - L[i * kMaxAssets + m] * L[k * kMaxAssets + m];
      L[i * kMaxAssets + k] = i == k ? sqrt(s > 0.0 ? s : 0.0) : s / L[k * kMaxAssets + k];
    }
}

template <int A, bool HW, int MODE>
__global__ __launch_bounds__(kBThreads) void basket_general_kernel(BasketArgs a, BasketGeneralArgs g,
                                                                   double* __restrict__ prices) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  extern __shared__ double lds[];  // kBGeneralHead doubles of scratch, then (kBPriceLds) the parked block
  double* Ld = lds + kBWaves * kBPriceSums;     // [8][8]
  double* wsum = Ld + kMaxAssets * kMaxAssets;  // [kBWaves][A]
  double* tot = wsum + kBWaves * kMaxAssets;    // [A]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T = a.T;
  const int64_t P = a.P;
  const int64_t P4 = (P + 3) & ~int64_t{3};  // the parked block's row length
  v4f* park = reinterpret_cast<v4f*>(lds + kBGeneralHead);

  const double* c = a.contracts + b * (3 * A + 4);
  const double Tm = c[1], r = c[2], rho = c[3];
  if (tid == 0) cholesky_general(A, rho, g.corr ? g.corr + b * g.corr_stride : nullptr, Ld);
  __syncthreads();
  // per-asset log2-unit coefficients, as basket_kernel
  const double dt = Tm / static_cast<double>(T);
  const double sq = sqrt(dt);
  constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
  float ca[A], x0[A], Lb[A][A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double drift = r - d - 0.5 * v * v;
    ca[i] = static_cast<float>(drift * dt * kBLog2e);
    const double bi = v * sq * kBLog2e * zscale;
    x0[i] = static_cast<float>(c[4 + i]);
#pragma unroll
    for (int k = 0; k < A; ++k) Lb[i][k] = k <= i ? static_cast<float>(bi * Ld[i * kMaxAssets + k]) : 0.0f;
  }
  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);

  // payoff constants (basket_price_kernel's) and the weights
  const float Tf = static_cast<float>(Tm);
  const float df = math::exp_any(static_cast<float>(-r) * Tf);
  const float Kf = static_cast<float>(c[0]);
  float wt[A];  // the same for every lane: kept in scalar registers, beside the path loop's vector ones
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const float w = g.weights ? static_cast<float>(g.weights[b * g.weights_stride + i]) : static_cast<float>(1.0 / A);
    wt[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, w)));
  }
  auto forward = [&](int i) {
    return static_cast<float>(c[4 + i]) * math::exp_any(static_cast<float>(r - c[4 + A + i]) * Tf);
  };
  auto valid_paths = [&](int64_t chunk) {  // how many of the lane's 4 values of this chunk are paths (< P)
    const int64_t left = P - chunk - kBPaths * static_cast<int64_t>(tid);
    return static_cast<int>(left <= 0 ? 0 : (left >= kBPaths ? kBPaths : left));
  };
  auto simulate = [&](int64_t chunk, float(&x)[A][kBPaths]) {
    PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
    basket_lane_paths<A, HW>(s, ca, x0, Lb, T, x);
  };
  double v[kBPriceSums];
#pragma unroll
  for (int i = 0; i < kBPriceSums; ++i) v[i] = 0.0;
  auto payoffs = [&](const float(&x)[A][kBPaths], int nvalid, const float(&sc)[A]) {
    auto pay = [&](float diff) { return static_cast<double>(df * (diff > 0.0f ? diff : 0.0f)); };
#pragma unroll
    for (int j = 0; j < kBPaths; ++j) {
      if (j < nvalid) {
        float bk = 0.0f, mx = 0.0f, mn = 0.0f;
#pragma unroll
        for (int i = 0; i < A; ++i) {
          const float xs = x[i][j] * sc[i];
          bk = bk + wt[i] * xs;
          mx = i == 0 || xs > mx ? xs : mx;
          mn = i == 0 || xs < mn ? xs : mn;
        }
        const double p[6] = {pay(Kf - bk), pay(bk - Kf), pay(Kf - mx), pay(mx - Kf), pay(Kf - mn), pay(mn - Kf)};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          v[i] += p[i];
          v[6 + i] += p[i] * p[i];
        }
        v[12] += static_cast<double>(bk);
        v[13] += static_cast<double>(mx);
        v[14] += static_cast<double>(mn);
        v[15] += bk < Kf ? 1.0 : 0.0;
      }
    }
  };

  // pass 1: the terminal sums (RAW: and the payoffs, scale 1; lds: and the parked values)
  float sc[A];
#pragma unroll
  for (int i = 0; i < A; ++i) sc[i] = 1.0f;
  double acc[A];
#pragma unroll
  for (int i = 0; i < A; ++i) acc[i] = 0.0;
  for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
    const int nvalid = valid_paths(chunk);
    if (nvalid > 0) {
      float x[A][kBPaths];
      simulate(chunk, x);
#pragma unroll
      for (int i = 0; i < A; ++i) {
        float p = 0.0f;
#pragma unroll
        for (int j = 0; j < kBPaths; ++j) p += j < nvalid ? x[i][j] : 0.0f;
        acc[i] += static_cast<double>(p);
      }
      if constexpr (MODE == kBPriceRaw) payoffs(x, nvalid, sc);
      if constexpr (MODE == kBPriceLds) {
        // slot (chunk + 4 tid) / 4 of row i: chunk + 4 tid < P, so the slot ends at or before P4
#pragma unroll
        for (int i = 0; i < A; ++i)
          park[(i * P4 + chunk) / kBPaths + tid] = v4f{x[i][0], x[i][1], x[i][2], x[i][3]};
      }
    }
  }
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double w = bwave_sum(acc[i]);
    if (lane == 0) wsum[wave * A + i] = w;
  }
  __syncthreads();
  if (tid < A) {
    double sum = 0.0;
    for (int w = 0; w < kBWaves; ++w) sum += wsum[w * A + tid];
    tot[tid] = sum;
    if (a.terminal_sum) a.terminal_sum[b * A + tid] = sum;
  }
  if constexpr (MODE != kBPriceRaw) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < A; ++i) sc[i] = forward(i) / static_cast<float>(tot[i] / static_cast<double>(P));
    // pass 2: the payoffs of the lane's own values, parked or simulated again
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float x[A][kBPaths];
        if constexpr (MODE == kBPriceLds) {
#pragma unroll
          for (int i = 0; i < A; ++i) {
            const v4f q = park[(i * P4 + chunk) / kBPaths + tid];
#pragma unroll
            for (int j = 0; j < kBPaths; ++j) x[i][j] = q[j];
          }
        } else {
          simulate(chunk, x);
        }
        payoffs(x, nvalid, sc);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kBPriceSums; ++i) {
    const double w = bwave_sum(v[i]);
    if (lane == 0) lds[wave * kBPriceSums + i] = w;
  }
  __syncthreads();
  auto total = [&](int i) {
    double t = 0.0;
    for (int w = 0; w < kBWaves; ++w) t += lds[w * kBPriceSums + i];
    return t;
  };
  const double n = static_cast<double>(P);
  double* out = prices + b * SMC_BASKET_PRICE_COLS;
  if (tid < 6) {  // a payoff's mean and standard error
    const double m = total(tid) / n;
    double se = 0.0;
    if (P > 1) {
      const double var = total(6 + tid) - n * m * m;
      se = sqrt((var > 0.0 ? var : 0.0) / (n - 1.0) / n);
    }
    out[tid] = m;
    out[6 + tid] = se;
  } else if (tid >= 12 && tid < kBPriceSums) {  // means of bk, mx, mn; the exercise share
    out[tid] = total(tid) / n;
  } else if (tid == kBPriceSums) {  // intrinsic basket put / call on Fb = ((0 + w_0 F_0) + w_1 F_1) + ...
    float fb = 0.0f;
#pragma unroll
    for (int i = 0; i < A; ++i) fb = fb + wt[i] * forward(i);
    const float ip = Kf - fb, ic = fb - Kf;
    out[16] = static_cast<double>(df * (ip > 0.0f ? ip : 0.0f));
    out[17] = static_cast<double>(df * (ic > 0.0f ? ic : 0.0f));
  }
}

template <int... I, typename F>
__device__ __forceinline__ void basket_static_for(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}

// ---- path-dependent basket pricing: basket_path_kernel (smc_basket_price_paths) ---------------------
// basket_general_kernel's front end (contract rows, streams, weights, cholesky_general, step coefficients, the
// 512-lane workgroup per contract, 4 paths per lane and 2048-path chunk, validity for any P >= 1) with
// path_price_kernel's per-row hook on basket_lane_paths: every monitoring date t of the [A][T][P] block the
// training call would store is seen in registers as xs_it = x_it s_it (s = 1 under RAW), and gives the basket
// level b_t = ((0 + w_0 xs_0t) + w_1 xs_1t) + ... and the worst level m_t = min_i xs_it.  Each path keeps the
// running sum, maximum and minimum of b_t and two knocked flags (b_t <= lower || b_t >= upper; m_t <= worst_lower).
// From those come ten payoffs per path (Asian, knock-out, lookback, worst-of knock-out, European; put and call) and
// kBPathSums f64 sums per contract: the payoffs, their squares, the average, the two knocked counts, the maximum and
// the minimum.  There is no parked mode: A T P values do not fit in LDS.
//   RAW        one simulation per column group; the terminal sums ride along with the first one as per-lane f64
//              accumulators in dynamic LDS ([A][512], lane tid touches column tid only: no registers beside the
//              payoff sums).
//   NORMALIZE  first the A T row sums in basket_general_kernel's tot_i order (the lane's valid values left to right
//              in f32 from 0, then f64 per lane over its chunks, butterfly, waves 0..7): the per-lane accumulators
//              of R = dates * A rows live in dynamic LDS ([R][512] doubles), and the T dates are covered in sweeps
//              of `dates` whole time rows, each re-simulating from row 0 to its last row; a row's sum lies in one
//              sweep, so a sweep boundary changes no order.  The A T scales stay in LDS as f32 ([T][A]); the
//              payoff simulations re-create the same streams and apply them.
// Column groups: 25 f64 sums and 14 registers of per-path state fit beside the 4 A path values for A <= 4 (one
// payoff simulation).  From A = 5 on the columns are taken in three groups over three simulations: {Asian,
// European}, {knock-out, worst-of knock-out}, {lookback}; a sum belongs to one group and keeps its order, so the
// European columns stay the price call's bit for bit.
constexpr int kBPathSums = 25;  // 10 payoffs, their squares, avg, count(ko), count(wko), mxb, mnb
// scratch at the head of the dynamic LDS: payoff-sum partials [kBWaves][kBPathSums] and the Cholesky factor [8][8]
// (f64; 2112 B)
constexpr int kBPathHead = kBWaves * kBPathSums + kMaxAssets * kMaxAssets;
constexpr size_t kBPathScratch = kBPathHead * sizeof(double);
constexpr size_t kBPathAccRow = kBThreads * sizeof(double);  // one row of per-lane row-sum accumulators
constexpr size_t kBPathLdsBytes = 144 * 1024;                // dynamic LDS a workgroup may take
constexpr int basket_path_groups(int A) { return A <= 4 ? 1 : 3; }
// payoff family of a sum: 0 Asian, 1 knock-out, 2 lookback, 3 worst-of knock-out, 4 European
constexpr int basket_path_family(int sum) {
  return sum < 20 ? (sum % 10) / 2 : (sum == 20 ? 0 : (sum == 21 ? 1 : (sum == 22 ? 3 : 2)));
}
constexpr bool basket_path_in_group(int A, int group, int sum) {
  if (basket_path_groups(A) == 1) return true;
  const int f = basket_path_family(sum);
  return group == 0 ? (f == 0 || f == 4) : (group == 1 ? (f == 1 || f == 3) : f == 2);
}

template <int A, bool HW, bool NORMALIZE>
__global__ __launch_bounds__(kBThreads) void basket_path_kernel(BasketArgs a, BasketGeneralArgs g,
                                                                const double* __restrict__ barriers,
                                                                double* __restrict__ prices, int sweep_dates) {
  constexpr int NG = basket_path_groups(A);
  // kBPathHead doubles of scratch; NORMALIZE: then the A T scales (f32, padded to 8 B); then the accumulator rows
  // ([sweep_dates * A][512] under NORMALIZE, [A][512] under RAW)
  extern __shared__ double lds[];
  double* Ld = lds + kBWaves * kBPathSums;  // [8][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T = a.T;
  const int64_t P = a.P;
  float* scales = reinterpret_cast<float*>(lds + kBPathHead);  // [T][A]
  double* acc = lds + kBPathHead + (NORMALIZE ? (static_cast<size_t>(A) * T * sizeof(float) + 7) / 8 : 0);

  const double* c = a.contracts + b * (3 * A + 4);
  const double Tm = c[1], r = c[2], rho = c[3];
  if (tid == 0) cholesky_general(A, rho, g.corr ? g.corr + b * g.corr_stride : nullptr, Ld);
  __syncthreads();
  // per-asset log2-unit coefficients, as basket_kernel
  const double dt = Tm / static_cast<double>(T);
  const double sq = sqrt(dt);
  constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
  float ca[A], x0[A], Lb[A][A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double drift = r - d - 0.5 * v * v;
    ca[i] = static_cast<float>(drift * dt * kBLog2e);
    const double bi = v * sq * kBLog2e * zscale;
    x0[i] = static_cast<float>(c[4 + i]);
#pragma unroll
    for (int k = 0; k < A; ++k) Lb[i][k] = k <= i ? static_cast<float>(bi * Ld[i * kMaxAssets + k]) : 0.0f;
  }
  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);

  auto uniform = [](float f) {  // the same for every lane: kept in a scalar register
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, f)));
  };
  auto valid_paths = [&](int64_t chunk) {  // how many of the lane's 4 values of this chunk are paths (< P)
    const int64_t left = P - chunk - kBPaths * static_cast<int64_t>(tid);
    return static_cast<int>(left <= 0 ? 0 : (left >= kBPaths ? kBPaths : left));
  };
  // the lane's valid values of one asset and row, left to right in f32 from 0, onto its own f64 accumulator
  auto add_row = [&](double* slot, const float(&xr)[kBPaths], int nvalid) {
    float p = 0.0f;
#pragma unroll
    for (int j = 0; j < kBPaths; ++j) p += j < nvalid ? xr[j] : 0.0f;
    *slot += static_cast<double>(p);
  };
  // rows [0, nrows) of acc: wave butterfly into lane 0's own slot; after the barrier thread q totals waves 0..7
  auto reduce_rows = [&](int nrows) {
    for (int q = 0; q < nrows; ++q) {
      const double w = bwave_sum(acc[q * kBThreads + tid]);
      if (lane == 0) acc[q * kBThreads + tid] = w;
    }
    __syncthreads();
  };
  auto row_total = [&](int q) {
    double sum = 0.0;
    for (int w = 0; w < kBWaves; ++w) sum += acc[q * kBThreads + w * 64];
    return sum;
  };

  if constexpr (NORMALIZE) {
    for (int t0 = 0; t0 < T; t0 += sweep_dates) {
      const int nd = T - t0 < sweep_dates ? T - t0 : sweep_dates;
      const int nrows = nd * A;  // <= the rows the host sized acc for
      for (int q = 0; q < nrows; ++q) acc[q * kBThreads + tid] = 0.0;
      for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
        const int nvalid = valid_paths(chunk);
        if (nvalid > 0) {
          PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
          float x[A][kBPaths];
          basket_lane_paths<A, HW>(s, ca, x0, Lb, t0 + nd, x, [&](const float(&xr)[A][kBPaths], int t) {
            if (t >= t0) {  // t < t0 + nd: date t - t0 of this sweep, the lane's own column
              double* row = acc + static_cast<size_t>(t - t0) * A * kBThreads + tid;
#pragma unroll
              for (int i = 0; i < A; ++i) add_row(row + i * kBThreads, xr[i], nvalid);
            }
          });
        }
      }
      reduce_rows(nrows);
      if (tid < nrows) {
        const double sum = row_total(tid);
        const int idx = t0 * A + tid;  // t * A + i
        scales[idx] = static_cast<float>(sum / static_cast<double>(P));  // the row mean, for now
        if (a.terminal_sum && idx >= (T - 1) * A) a.terminal_sum[b * A + (idx - (T - 1) * A)] = sum;
      }
      __syncthreads();  // the accumulators are free for the next sweep
    }
    for (int idx = tid; idx < A * T; idx += kBThreads) {
      const int t = idx / A, i = idx - t * A;
      const double tau = t == T - 1 ? Tm : static_cast<double>(t + 1) * dt;
      const float F = static_cast<float>(c[4 + i]) * math::exp_any(static_cast<float>(r - c[4 + A + i]) * static_cast<float>(tau));
      scales[idx] = F / scales[idx];
    }
    __syncthreads();
  }

  // payoff constants (basket_general_kernel's), the weights and the barriers
  const float Tf = static_cast<float>(Tm);
  const float df = math::exp_any(static_cast<float>(-r) * Tf);
  const float Kf = static_cast<float>(c[0]);
  const float steps = static_cast<float>(T);
  float wt[A];
#pragma unroll
  for (int i = 0; i < A; ++i)
    wt[i] = uniform(g.weights ? static_cast<float>(g.weights[b * g.weights_stride + i]) : static_cast<float>(1.0 / A));
  const float inf = __builtin_huge_valf();
  const float lower = uniform(barriers ? static_cast<float>(barriers[3 * b]) : -inf);
  const float upper = uniform(barriers ? static_cast<float>(barriers[3 * b + 1]) : inf);
  const float wlower = uniform(barriers ? static_cast<float>(barriers[3 * b + 2]) : -inf);
  auto pay = [&](float diff) { return static_cast<double>(df * (diff > 0.0f ? diff : 0.0f)); };
  // basket and worst level of path j at row t
  auto level = [&](const float(&xr)[A][kBPaths], const float(&sc)[A], int j, float& bt, float& mt) {
    bt = 0.0f;
    mt = 0.0f;
#pragma unroll
    for (int i = 0; i < A; ++i) {
      const float xs = NORMALIZE ? xr[i][j] * sc[i] : xr[i][j];
      bt = bt + wt[i] * xs;
      mt = i == 0 || xs < mt ? xs : mt;
    }
  };
  auto row_scales = [&](int t, float(&sc)[A]) {
#pragma unroll
    for (int i = 0; i < A; ++i) sc[i] = NORMALIZE ? scales[t * A + i] : 1.0f;
  };

  basket_static_for(std::make_integer_sequence<int, NG>{}, [&](auto tag) {
    constexpr int G = decltype(tag)::value;
    constexpr bool ASIAN = basket_path_in_group(A, G, 0), KO = basket_path_in_group(A, G, 2),
                   LOOK = basket_path_in_group(A, G, 4), WORST = basket_path_in_group(A, G, 6);
    constexpr bool TERMINAL = !NORMALIZE && G == 0;  // RAW: the terminal sums ride along with the first group
    double v[kBPathSums];
#pragma unroll
    for (int k = 0; k < kBPathSums; ++k) v[k] = 0.0;
    if constexpr (TERMINAL)
      for (int i = 0; i < A; ++i) acc[i * kBThreads + tid] = 0.0;
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float sa[kBPaths], mxb[kBPaths], mnb[kBPaths];
        unsigned ko = 0, wko = 0;
#pragma unroll
        for (int j = 0; j < kBPaths; ++j) {
          sa[j] = 0.0f;
          mxb[j] = -inf;
          mnb[j] = inf;
        }
        PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
        float x[A][kBPaths];
        basket_lane_paths<A, HW>(s, ca, x0, Lb, T, x, [&](const float(&xr)[A][kBPaths], int t) {
          float sc[A];
          row_scales(t, sc);
#pragma unroll
          for (int j = 0; j < kBPaths; ++j) {
            float bt, mt;
            level(xr, sc, j, bt, mt);
            if constexpr (ASIAN) sa[j] = sa[j] + bt;
            if constexpr (LOOK) {
              mxb[j] = bt > mxb[j] ? bt : mxb[j];
              mnb[j] = bt < mnb[j] ? bt : mnb[j];
            }
            if constexpr (KO) ko |= (bt <= lower || bt >= upper) ? (1u << j) : 0u;
            if constexpr (WORST) wko |= mt <= wlower ? (1u << j) : 0u;
          }
        });
        if constexpr (TERMINAL) {
#pragma unroll
          for (int i = 0; i < A; ++i) add_row(acc + i * kBThreads + tid, x[i], nvalid);
        }
        float sc[A];
        row_scales(T - 1, sc);
#pragma unroll
        for (int j = 0; j < kBPaths; ++j) {
          if (j < nvalid) {
            float bl, ml;  // the hook's values of row T - 1
            level(x, sc, j, bl, ml);
            const float avg = sa[j] / steps;
            const bool kb = (ko >> j) & 1u, kw = (wko >> j) & 1u;
            const double put = pay(Kf - bl), call = pay(bl - Kf), wput = pay(Kf - ml), wcall = pay(ml - Kf);
            const double p[10] = {pay(Kf - avg),    pay(avg - Kf),    kb ? 0.0 : put,  kb ? 0.0 : call, pay(Kf - mnb[j]),
                                  pay(mxb[j] - Kf), kw ? 0.0 : wput, kw ? 0.0 : wcall, put,             call};
#pragma unroll
            for (int k = 0; k < 10; ++k) {
              if constexpr (NG == 1) {
                v[k] += p[k];
                v[10 + k] += p[k] * p[k];
              } else if (basket_path_in_group(A, G, k)) {
                v[k] += p[k];
                v[10 + k] += p[k] * p[k];
              }
            }
            if constexpr (ASIAN) v[20] += static_cast<double>(avg);
            if constexpr (KO) v[21] += kb ? 1.0 : 0.0;
            if constexpr (WORST) v[22] += kw ? 1.0 : 0.0;
            if constexpr (LOOK) {
              v[23] += static_cast<double>(mxb[j]);
              v[24] += static_cast<double>(mnb[j]);
            }
          }
        }
      }
    }
    // the group's sums: wave butterfly into its own slots of the partials (the groups' slots are disjoint)
#pragma unroll
    for (int k = 0; k < kBPathSums; ++k) {
      if (basket_path_in_group(A, G, k)) {
        const double w = bwave_sum(v[k]);
        if (lane == 0) lds[wave * kBPathSums + k] = w;
      }
    }
    if constexpr (TERMINAL) {
      reduce_rows(A);
      if (tid < A && a.terminal_sum) a.terminal_sum[b * A + tid] = row_total(tid);
    }
  });
  __syncthreads();
  // waves 0..7, sum k totalled by thread k alone (path_price_kernel's way)
  auto total = [&](int k) {
    double t2 = 0.0;
    for (int w = 0; w < kBWaves; ++w) t2 += lds[w * kBPathSums + k];
    return t2;
  };
  const double n = static_cast<double>(P);
  double* out = prices + b * SMC_BASKET_PATH_COLS;
  if (tid < 10) {  // a payoff's mean and standard error
    const double m = total(tid) / n;
    double se = 0.0;
    if (P > 1) {
      const double var = total(10 + tid) - n * m * m;
      se = sqrt((var > 0.0 ? var : 0.0) / (n - 1.0) / n);
    }
    out[tid] = m;
    out[10 + tid] = se;
  } else if (tid >= 20 && tid < kBPathSums) {
    out[tid] = total(tid) / n;
  }
}

// ---- batched basket Greeks: basket_greeks_kernel (smc_basket_greeks) -----------------------------
// basket_price_kernel's geometry, streams, chunk / validity handling, modes and sum orders (restated, not
// shared: basket_price_kernel's registers stay as they are; the path loop is basket_lane_paths, which only the
// price kernel and this one call).  The A terminal values of a path give its log returns L_i = log(x_i / X0_i)
// and, through G = (dLc / drho) Lc^-1, the derivative c_i of asset i's correlated Brownian sum with respect to
// the equicorrelation parameter: every pathwise derivative of the equal-weight basket put and call follows (the
// table of include/spectralmc_hip.h).  NT = 4A + 8 per-path f32 terms (delta and vega per asset,
// rho, theta, correlation, price; put and call), each cast to f64 and added with its square.
// Registers: 2 NT f64 accumulators per lane do not fit beside the path loop from A = 5 on, so the terms are
// taken basket_greek_pass_terms(A) at a time in payoff passes over the parked (lds) or re-simulated (raw,
// replay) values, after a pass for the terminal sums alone and (NORMALIZE) one for sxl and sxc; a sum belongs to
// one pass, so it keeps its one order and lds and replay stay bit-identical.  The per-asset constants of the table live in LDS as f32 (written once per contract by the
// threads below A, read back by every lane), not in registers.
constexpr int basket_greek_terms(int A) { return 4 * A + 8; }
constexpr int basket_greek_pass_terms(int A) { return A <= 4 ? basket_greek_terms(A) : 8; }
constexpr int kBGreekRed = 2 * basket_greek_terms(4);  // the widest pass: 24 terms and their squares
constexpr int kBGreekFc = 8;                           // f32 constants per asset: s, ix0, cv, av, aT, ac, g0
// scratch at the head of the dynamic LDS (f64): pass-sum partials [kBWaves][kBGreekRed], Lc, dLc / drho and G
// [8][8] each, pass-1 partials [kBWaves][3][8] and totals [3][8] (tot, sxl, sxc), then the f32 constants
// [8][kBGreekFc] and g [8][8] (6848 B, a multiple of 16)
constexpr int kBGreekHead = kBWaves * kBGreekRed + 3 * kMaxAssets * kMaxAssets + kBWaves * 3 * kMaxAssets +
                            3 * kMaxAssets + (kMaxAssets * kBGreekFc + kMaxAssets * kMaxAssets) / 2;
constexpr size_t kBGreekScratch = kBGreekHead * sizeof(double);

// d Lc / d rho of the Banachiewicz recursion of cholesky_equicorr (the derivative of each of its statements, in
// its order), then G = dLc Lc^-1 row by row from the last column (G Lc = dLc; G is lower triangular).  f64, one
// thread, matrices in LDS with row stride 8.
__device__ void cholesky_equicorr_drho(int A, const double* L, double* dL, double* G) {
  for (int i = 0; i < A; ++i)
    for (int k = 0; k <= i; ++k) {
      double ds = i == k ? 0.0 : 1.0;
      for (int m = 0; m < k; ++m)
        ds = ds - (dL[i * kMaxAssets + m] * L[k * kMaxAssets + m] + L[i * kMaxAssets + m] * dL[k * kMaxAssets + m]);
      dL[i * kMaxAssets + k] = i == k ? ds / (2.0 * L[i * kMaxAssets + i])
                                      : (ds - L[i * kMaxAssets + k] * dL[k * kMaxAssets + k]) / L[k * kMaxAssets + k];
    }
  for (int i = 0; i < A; ++i)
    for (int k = i; k >= 0; --k) {
      double g = dL[i * kMaxAssets + k];
      for (int m = k + 1; m <= i; ++m) g = g - G[i * kMaxAssets + m] * L[m * kMaxAssets + k];
      G[i * kMaxAssets + k] = g / L[k * kMaxAssets + k];
    }
}

template <bool HW>
__device__ __forceinline__ float basket_greeks_log(float x, float x0) {
  const float q = x / x0;
  if constexpr (HW) return math::hw_log(q);
  else return math::log_pos(q);
}

template <int A, bool HW, int MODE>
__global__ __launch_bounds__(kBThreads) void basket_greeks_kernel(BasketArgs a, double* __restrict__ greeks,
                                                                  double* __restrict__ sums) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  constexpr int NT = basket_greek_terms(A);       // per-path terms
  constexpr int TP = basket_greek_pass_terms(A);  // terms per payoff pass
  constexpr int NP = (NT + TP - 1) / TP;          // payoff passes
  constexpr int NG = NT - 2;                      // Greek columns n = 4A + 6
  extern __shared__ double lds[];  // kBGreekHead doubles of scratch, then (kBPriceLds) the parked block
  double* Ld = lds + kBWaves * kBGreekRed;        // [8][8]
  double* dLd = Ld + kMaxAssets * kMaxAssets;     // [8][8]
  double* Gd = dLd + kMaxAssets * kMaxAssets;     // [8][8]
  double* wsum = Gd + kMaxAssets * kMaxAssets;    // [kBWaves][3][8]
  double* tot = wsum + kBWaves * 3 * kMaxAssets;  // [3][8]: tot, sxl, sxc
  float* fc = reinterpret_cast<float*>(tot + 3 * kMaxAssets);  // [8][kBGreekFc]
  float* gk = fc + kMaxAssets * kBGreekFc;        // [8][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T = a.T;
  const int64_t P = a.P;
  const int64_t P4 = (P + 3) & ~int64_t{3};  // the parked block's row length
  v4f* park = reinterpret_cast<v4f*>(lds + kBGreekHead);

  const double* c = a.contracts + b * (3 * A + 4);
  const double Tm = c[1], r = c[2], rho = c[3];
  if (tid == 0) {
    cholesky_equicorr(A, rho, Ld);
    cholesky_equicorr_drho(A, Ld, dLd, Gd);
  }
  __syncthreads();
  // per-asset log2-unit coefficients, as basket_kernel
  const double dt = Tm / static_cast<double>(T);
  const double sq = sqrt(dt);
  constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
  float ca[A], x0[A], Lb[A][A];
  bool anyv0 = false;
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double drift = r - d - 0.5 * v * v;
    ca[i] = static_cast<float>(drift * dt * kBLog2e);
    const double bi = v * sq * kBLog2e * zscale;
    x0[i] = static_cast<float>(c[4 + i]);
    anyv0 = anyv0 || v == 0.0;
#pragma unroll
    for (int k = 0; k < A; ++k) Lb[i][k] = k <= i ? static_cast<float>(bi * Ld[i * kMaxAssets + k]) : 0.0f;
  }
  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);

  // payoff constants (basket_price_kernel's) and the scalar constants of the table
  const float Tf = static_cast<float>(Tm);
  const float df = math::exp_any(static_cast<float>(-r) * Tf);
  const float Kf = static_cast<float>(c[0]);
  const float wA = static_cast<float>(1.0 / A);
  const float cT = Tm == 0.0 ? 0.0f : static_cast<float>(1.0 / (2.0 * Tm));
  const float crho = df * (Tf * Kf);
  const float rr = static_cast<float>(r);
  auto forward = [&](int i) {
    return static_cast<float>(c[4 + i]) * math::exp_any(static_cast<float>(r - c[4 + A + i]) * Tf);
  };
  // the constants that need no sum: g_ik (thread 8 i + k), and per asset ix0, cv, g0 and RAW's s, av, aT, ac.
  // A deterministic asset (some v == 0) leaves no driver to recover: g = g0 = 0, the correlation columns NaN.
  if (tid < kMaxAssets * kMaxAssets) {
    const int i = tid >> 3, k = tid & 7;
    float g = 0.0f;
    if (i < A && k <= i && !anyv0)
      g = static_cast<float>(c[4 + 2 * A + i] * Gd[i * kMaxAssets + k] / c[4 + 2 * A + k]);
    gk[tid] = g;
  }
  if (tid < A) {
    const int i = tid;
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double mu = r - d - 0.5 * v * v;
    double gs = 0.0;
    if (!anyv0)
      for (int k = 0; k <= i; ++k) {
        const double vk = c[4 + 2 * A + k];
        const double muk = r - c[4 + A + k] - 0.5 * vk * vk;
        gs = gs + Gd[i * kMaxAssets + k] * muk * Tm / vk;
      }
    float* f = fc + i * kBGreekFc;
    f[0] = 1.0f;
    f[1] = static_cast<float>(1.0 / c[4 + i]);
    f[2] = v == 0.0 ? 0.0f : static_cast<float>(1.0 / v);
    f[3] = v == 0.0 ? 0.0f : static_cast<float>(-mu * Tm / v - v * Tm);
    f[4] = static_cast<float>(mu / 2.0);
    f[5] = 0.0f;
    f[6] = anyv0 ? 0.0f : static_cast<float>(-(v * gs));
  }
  __syncthreads();

  auto valid_paths = [&](int64_t chunk) {  // how many of the lane's 4 values of this chunk are paths (< P)
    const int64_t left = P - chunk - kBPaths * static_cast<int64_t>(tid);
    return static_cast<int>(left <= 0 ? 0 : (left >= kBPaths ? kBPaths : left));
  };
  auto simulate = [&](int64_t chunk, float(&x)[A][kBPaths]) {
    PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
    basket_lane_paths<A, HW>(s, ca, x0, Lb, T, x);
  };
  // c_i = g0_i + sum_{k <= i} g_ik L_k in k order (every operation rounded)
  auto corr = [&](int i, const float(&L)[A]) {
    float ci = fc[i * kBGreekFc + 6];
#pragma unroll
    for (int k = 0; k < A; ++k)
      if (k <= i) ci = ci + gk[i * kMaxAssets + k] * L[k];
    return ci;
  };
  // terminal sums of one chunk in basket_price_kernel's order
  auto add_terminal = [&](const float(&x)[A][kBPaths], int nvalid, double(&acc)[A]) {
#pragma unroll
    for (int i = 0; i < A; ++i) {
      float p = 0.0f;
#pragma unroll
      for (int j = 0; j < kBPaths; ++j) p += j < nvalid ? x[i][j] : 0.0f;
      acc[i] += static_cast<double>(p);
    }
  };
  // a lane's partial of pass-1 sum q (0 tot, 1 sxl, 2 sxc) through the wave butterfly; finish_sums then adds
  // waves 0..7 of the first nq sums (the others are 0) and reports them
  auto wave_sums = [&](const double(&acc)[A], int q) {
#pragma unroll
    for (int i = 0; i < A; ++i) {
      const double w = bwave_sum(acc[i]);
      if (lane == 0) wsum[(wave * 3 + q) * kMaxAssets + i] = w;
    }
  };
  auto finish_sums = [&](int nq) {
    __syncthreads();
    if (tid < 3 * kMaxAssets) {
      const int q = tid >> 3, i = tid & 7;
      if (i < A) {
        double sum = 0.0;
        if (q < nq)
          for (int w = 0; w < kBWaves; ++w) sum += wsum[(w * 3 + q) * kMaxAssets + i];
        tot[tid] = sum;
        if (sums) sums[b * (3 * A) + q * A + i] = sum;
      }
    }
    __syncthreads();
  };
  // One pass over the paths for the sums that come before the payoffs: TOT the terminal sums (the first pass
  // over the paths: it simulates and, in the lds mode, parks), XLXC sxl_i = sum f64(x_i L_i) and
  // sxc_i = sum f64(x_i c_i).  A <= 4 takes all three together; from A = 5 on the 3A accumulators do not fit
  // beside the path loop, and TOT goes first, alone.
  auto sum_pass = [&](auto tot_tag, auto xlxc_tag) {
    constexpr bool TOT = decltype(tot_tag)::value, XLXC = decltype(xlxc_tag)::value;
    double acc[3][A];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int i = 0; i < A; ++i) acc[q][i] = 0.0;
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float x[A][kBPaths];
        if constexpr (MODE == kBPriceLds && !TOT) {  // the lane's own values: no barrier needed
#pragma unroll
          for (int i = 0; i < A; ++i) {
            const v4f q = park[(i * P4 + chunk) / kBPaths + tid];
#pragma unroll
            for (int j = 0; j < kBPaths; ++j) x[i][j] = q[j];
          }
        } else {
          simulate(chunk, x);
        }
        if constexpr (TOT) add_terminal(x, nvalid, acc[0]);
        if constexpr (XLXC) {
#pragma unroll
          for (int j = 0; j < kBPaths; ++j) {
            if (j < nvalid) {
              if constexpr (A > 4) asm volatile("" ::: "memory");  // the LDS constants are read per path, not kept
              float L[A];
#pragma unroll
              for (int i = 0; i < A; ++i) L[i] = basket_greeks_log<HW>(x[i][j], x0[i]);
#pragma unroll
              for (int i = 0; i < A; ++i) {
                acc[1][i] += static_cast<double>(x[i][j] * L[i]);
                acc[2][i] += static_cast<double>(x[i][j] * corr(i, L));
              }
            }
          }
        }
        if constexpr (MODE == kBPriceLds && TOT) {
          // slot (chunk + 4 tid) / 4 of row i: chunk + 4 tid < P, so the slot ends at or before P4
#pragma unroll
          for (int i = 0; i < A; ++i)
            park[(i * P4 + chunk) / kBPaths + tid] = v4f{x[i][0], x[i][1], x[i][2], x[i][3]};
        }
      }
    }
    if constexpr (TOT) wave_sums(acc[0], 0);
    if constexpr (XLXC) {
      wave_sums(acc[1], 1);
      wave_sums(acc[2], 2);
    }
  };
  constexpr bool kSplitSums = A > 4;
  using yes = std::true_type;
  using no = std::false_type;

  if constexpr (MODE != kBPriceRaw) {
    if constexpr (kSplitSums) {
      sum_pass(yes{}, no{});
      sum_pass(no{}, yes{});
    } else {
      sum_pass(yes{}, yes{});
    }
    finish_sums(3);
    if (tid < A) {  // the constants that move with the sums
      const int i = tid;
      const double v = c[4 + 2 * A + i], rd = r - c[4 + A + i];
      const double lbar = tot[kMaxAssets + i] / tot[i];
      float* f = fc + i * kBGreekFc;
      f[0] = forward(i) / static_cast<float>(tot[i] / static_cast<double>(P));
      f[3] = v == 0.0 ? 0.0f : static_cast<float>(-lbar / v);
      f[4] = Tm == 0.0 ? static_cast<float>(rd) : static_cast<float>(-lbar / (2.0 * Tm) + rd);
      f[5] = static_cast<float>(-tot[2 * kMaxAssets + i] / tot[i]);
    }
    __syncthreads();
  } else if constexpr (kSplitSums) {  // RAW from A = 5 on: the terminal sums in a pass of their own
    sum_pass(yes{}, no{});
    finish_sums(1);
  }

  // one path's terms of pass PASS (the table of the header), each cast to f64 and added with its square
  double v[2 * TP];
  auto payoffs = [&](auto tag, const float(&x)[A][kBPaths], int nvalid) {
    constexpr int T0 = decltype(tag)::value * TP;
#pragma unroll
    for (int j = 0; j < kBPaths; ++j) {
      if (j < nvalid) {
        // from A = 5 on the LDS constants are read again for every path: held across the path loop (where the
        // compiler hoists them to) they spill
        if constexpr (A > 4) asm volatile("" ::: "memory");
        float L[A], w[A], t[NT];
        float bs = 0.0f;
#pragma unroll
        for (int i = 0; i < A; ++i) {
          const float xs = x[i][j] * fc[i * kBGreekFc];
          bs = bs + xs;
          w[i] = (df * xs) * wA;
          L[i] = basket_greeks_log<HW>(x[i][j], x0[i]);
        }
        const float bk = bs * wA;
        const float dp = Kf - bk, dc = bk - Kf;
        const bool ip = dp > 0.0f, ic = dc > 0.0f;
        const float put = df * (ip ? dp : 0.0f), call = df * (ic ? dc : 0.0f);
        float sT = 0.0f, sC = 0.0f;
#pragma unroll
        for (int i = 0; i < A; ++i) {
          const float* f = fc + i * kBGreekFc;
          const float wd = w[i] * f[1];
          const float wv = w[i] * (L[i] * f[2] + f[3]);
          sT = sT + w[i] * (L[i] * cT + f[4]);
          sC = sC + w[i] * (corr(i, L) + f[5]);
          t[i] = ip ? -wd : 0.0f;
          t[A + i] = ic ? wd : 0.0f;
          t[2 * A + i] = ip ? -wv : 0.0f;
          t[3 * A + i] = ic ? wv : 0.0f;
        }
        t[4 * A] = ip ? -crho : 0.0f;
        t[4 * A + 1] = ic ? crho : 0.0f;
        t[4 * A + 2] = rr * put + (ip ? sT : 0.0f);
        t[4 * A + 3] = rr * call - (ic ? sT : 0.0f);
        t[4 * A + 4] = ip ? -sC : 0.0f;
        t[4 * A + 5] = ic ? sC : 0.0f;
        t[NG] = put;
        t[NG + 1] = call;
#pragma unroll
        for (int k = 0; k < TP; ++k) {
          if (T0 + k < NT) {
            const double d = static_cast<double>(t[T0 + k]);
            v[k] += d;
            v[TP + k] += d * d;
          }
        }
      }
    }
  };

  const double n = static_cast<double>(P);
  double* out = greeks + b * (2 * NG + 4);
#pragma unroll 1
  for (int pass = 0; pass < NP; ++pass) {
#pragma unroll
    for (int k = 0; k < 2 * TP; ++k) v[k] = 0.0;
    double acc[A];  // RAW, A <= 4: the terminal sums ride along with the one payoff pass
#pragma unroll
    for (int i = 0; i < A; ++i) acc[i] = 0.0;
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float x[A][kBPaths];
        if constexpr (MODE == kBPriceLds) {  // the lane's own values: no barrier needed
#pragma unroll
          for (int i = 0; i < A; ++i) {
            const v4f q = park[(i * P4 + chunk) / kBPaths + tid];
#pragma unroll
            for (int j = 0; j < kBPaths; ++j) x[i][j] = q[j];
          }
        } else {
          simulate(chunk, x);
        }
        if constexpr (MODE == kBPriceRaw && !kSplitSums) add_terminal(x, nvalid, acc);
        basket_static_for(std::make_integer_sequence<int, NP>{}, [&](auto tag) {
          if (NP == 1 || pass == decltype(tag)::value) payoffs(tag, x, nvalid);
        });
      }
    }
    if constexpr (MODE == kBPriceRaw && !kSplitSums) {
      wave_sums(acc, 0);
      finish_sums(1);  // sxl = sxc = 0
    }
    // the pass's sums: wave butterfly, waves 0..7, sum k totalled by thread k
#pragma unroll
    for (int k = 0; k < 2 * TP; ++k) {
      const double w = bwave_sum(v[k]);
      if (lane == 0) lds[wave * kBGreekRed + k] = w;
    }
    __syncthreads();
    const int term = pass * TP + tid;
    if (tid < TP && term < NT) {  // a term's mean and standard error
      auto total = [&](int k) {
        double t2 = 0.0;
        for (int w = 0; w < kBWaves; ++w) t2 += lds[w * kBGreekRed + k];
        return t2;
      };
      double m = total(tid) / n;
      double se = 0.0;
      if (P > 1) {
        const double var = total(TP + tid) - n * m * m;
        se = sqrt((var > 0.0 ? var : 0.0) / (n - 1.0) / n);
      }
      if (A > 1 && anyv0 && (term == 4 * A + 4 || term == 4 * A + 5)) m = se = __builtin_nan("");
      if (term < NG) {
        out[term] = m;
        out[NG + term] = se;
      } else {  // the prices: columns 2n, 2n + 1 and 2n + 2, 2n + 3
        out[NG + term] = m;
        out[NG + term + 2] = se;
      }
    }
    if (NP > 1) __syncthreads();  // the partials are rewritten by the next pass
  }
}

// ---- Greeks of the weighted, general-correlation basket: basket_greeks_general_kernel (smc_basket_greeks_general) ----
// basket_greeks_kernel with basket_general_kernel's two inputs (restated, not shared: the kernels above keep their
// registers): the factor is cholesky_general's, the basket is bk = ((0 + w_0 xs_0) + w_1 xs_1) + ... and a term's
// weight is (df xs_i) w_i.  The one correlation column becomes one per pair (j, k), k < j, in pack_correlation's
// order: d / dC_jk with the matrix kept symmetric, which is the derivative in the one entry the factor reads.  The
// drivers do not depend on C, so dW / dC_jk = G^jk W with G^jk = (dL / dC_jk) L^-1, and c_i^jk = g0_i^jk +
// sum_{m <= i} g_im^jk L_m is d ln x_i / dC_jk from the A terminal logs; rows i < j of G^jk are zero.  Thread q < np
// differentiates the Banachiewicz statements for pair q (seed 1 at (j, k)) and solves G L = dL in f64 (one thread per
// pair, not the one thread that factors: 28 pairs in turn would cost a contract some 10^4 dependent LDS round trips),
// then leaves g^q, g0^q (and later ac^q) in LDS as f32.  Under NORMALIZE every ac_i^jk follows per contract from the
// A (A + 1) / 2 moment sums M_im = sum_p f64(x_i L_m), m <= i (M_ii is basket_greeks_kernel's sxl_i).
// Terms per path: NT = 4A + 6 + A (A - 1); kernel order: the 4A + 4 delta, vega, rho and theta terms as columns, then
// (put, call) of pair 0, of pair 1, ..., then the two prices; they are taken basket_ggreek_pass_terms(A) at a time.
constexpr int basket_ggreek_pairs(int A) { return A * (A - 1) / 2; }
constexpr int basket_ggreek_terms(int A) { return 4 * A + 6 + 2 * basket_ggreek_pairs(A); }
constexpr int basket_ggreek_pass_terms(int A) { return A <= 3 ? basket_ggreek_terms(A) : (A == 4 ? 12 : 8); }
constexpr int kBGGRed = 2 * basket_ggreek_terms(3);     // the widest pass: 24 terms and their squares
constexpr int kBGGMaxPairs = basket_ggreek_pairs(kMaxAssets);                 // 28
constexpr int kBGGSums = kMaxAssets + kMaxAssets * (kMaxAssets + 1) / 2;      // tot [8], M packed [36]
constexpr int kBGGFc = 8;                               // f32 constants per asset: s, ix0, cv, av, aT
constexpr int kBGGPc = kMaxAssets * kMaxAssets + 2 * kMaxAssets;  // f32 per pair: g [8][8], g0 [8], ac [8]
// scratch at the head of the dynamic LDS (f64): pass-sum partials [kBWaves][kBGGRed], L [8][8], pass-1 partials
// [kBWaves][kBGGSums] and totals [kBGGSums], then the f32 constants [8][kBGGFc] and [28][kBGGPc]
// (15968 B, a multiple of 16)
constexpr int kBGGHead = kBWaves * kBGGRed + kMaxAssets * kMaxAssets + kBWaves * kBGGSums + kBGGSums +
                         (kMaxAssets * kBGGFc + kBGGMaxPairs * kBGGPc) / 2;
constexpr size_t kBGGScratch = kBGGHead * sizeof(double);
static_assert(kBGGScratch == 15968 && kBGGScratch % 16 == 0, "the header states the scratch bytes");

constexpr int basket_ggreek_pair_row(int q) {  // j of packed pair q = j (j - 1) / 2 + k
  int j = 1;
  while ((j + 1) * j / 2 <= q) ++j;
  return j;
}

// The f32 constants g^q, g0^q of pair q = (pj, pk) into its slice p of kBGGPc floats (ac^q = 0): dL / dC_jk by
// cholesky_equicorr_drho's statements with the seed 1 at (pj, pk) and 0 elsewhere, then G = dL L^-1 row by row.  f64,
// one thread, L in LDS with row stride 8.  dL is kept in the slice itself, packed row by row as f64 (36 of its 40
// doubles), and G one row at a time in registers: the rows are taken from the last to the first, so the floats of
// row i (doubles 4 i .. 4 i + 3, and 32 + i / 2 for g0) only overwrite dL rows already used (row i ends at double
// i (i + 1) / 2 + i <= 4 i + 3, and row 7 is used first).  Every loop is unrolled: all LDS offsets are constants.
template <int A>
__device__ __forceinline__ void cholesky_general_dpair(const double* L, int pj, int pk, const double* c, double r,
                                                       double Tm, bool anyv0, float* p) {
  double* dL = reinterpret_cast<double*>(p);
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int k = 0; k <= i; ++k) {
      double ds = (i == pj && k == pk) ? 1.0 : 0.0;
#pragma unroll
      for (int m = 0; m < k; ++m)
        ds = ds - (dL[i * (i + 1) / 2 + m] * L[k * kMaxAssets + m] + L[i * kMaxAssets + m] * dL[k * (k + 1) / 2 + m]);
      dL[i * (i + 1) / 2 + k] = i == k ? ds / (2.0 * L[i * kMaxAssets + i])
                                       : (ds - L[i * kMaxAssets + k] * dL[k * (k + 1) / 2 + k]) / L[k * kMaxAssets + k];
    }
#pragma unroll
  for (int i = A - 1; i >= 0; --i) {
    double G[A];
#pragma unroll
    for (int k = i; k >= 0; --k) {
      double g = dL[i * (i + 1) / 2 + k];
#pragma unroll
      for (int m = k + 1; m <= i; ++m) g = g - G[m] * L[m * kMaxAssets + k];
      G[k] = g / L[k * kMaxAssets + k];
    }
    asm volatile("" ::: "memory");  // the f32 stores below reuse the f64 row just read
    const double vi = c[4 + 2 * A + i];
    double gs = 0.0;
#pragma unroll
    for (int m = 0; m <= i; ++m) {
      const double vm = c[4 + 2 * A + m];
      const double mum = r - c[4 + A + m] - 0.5 * vm * vm;
      gs = gs + G[m] * mum * Tm / vm;
      p[i * kMaxAssets + m] = anyv0 ? 0.0f : static_cast<float>(vi * G[m] / vm);
    }
    p[kMaxAssets * kMaxAssets + i] = anyv0 ? 0.0f : static_cast<float>(-(vi * gs));
    asm volatile("" ::: "memory");
  }
#pragma unroll
  for (int i = 0; i < A; ++i) p[kMaxAssets * kMaxAssets + kMaxAssets + i] = 0.0f;
}

template <int A, bool HW, int MODE>
__global__ __launch_bounds__(kBThreads) void basket_greeks_general_kernel(BasketArgs a, BasketGeneralArgs g,
                                                                          double* __restrict__ greeks,
                                                                          double* __restrict__ sums) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  constexpr int NPR = basket_ggreek_pairs(A);      // pairs
  constexpr int NT = basket_ggreek_terms(A);       // per-path terms
  constexpr int TP = basket_ggreek_pass_terms(A);  // terms per payoff pass
  constexpr int NP = (NT + TP - 1) / TP;           // payoff passes
  constexpr int NG = NT - 2;                       // Greek columns n = 4A + 4 + 2 np
  constexpr int NM = A * (A + 1) / 2;              // moment sums
  constexpr int PT0 = 4 * A + 4;                   // the first pair term
  static_assert(2 * TP <= kBGGRed, "pass partials");
  extern __shared__ double lds[];  // kBGGHead doubles of scratch, then (kBPriceLds) the parked block
  double* Ld = lds + kBWaves * kBGGRed;           // [8][8]
  double* wsum = Ld + kMaxAssets * kMaxAssets;    // [kBWaves][kBGGSums]
  double* tot = wsum + kBWaves * kBGGSums;        // [kBGGSums]: tot [8], M_im at 8 + i (i + 1) / 2 + m
  float* fc = reinterpret_cast<float*>(tot + kBGGSums);  // [8][kBGGFc]
  float* pc = fc + kMaxAssets * kBGGFc;           // [28][kBGGPc]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T = a.T;
  const int64_t P = a.P;
  const int64_t P4 = (P + 3) & ~int64_t{3};  // the parked block's row length
  v4f* park = reinterpret_cast<v4f*>(lds + kBGGHead);

  const double* c = a.contracts + b * (3 * A + 4);
  const double Tm = c[1], r = c[2], rho = c[3];
  if (tid == 0) cholesky_general(A, rho, g.corr ? g.corr + b * g.corr_stride : nullptr, Ld);
  __syncthreads();
  bool anyv0 = false;
#pragma unroll
  for (int i = 0; i < A; ++i) anyv0 = anyv0 || c[4 + 2 * A + i] == 0.0;
  // Thread q < np: g^q, g0^q of its pair (ac^q = 0 until the sums are known).  A deterministic asset (some v == 0)
  // leaves no driver to recover: g = g0 = 0, the pair columns NaN.
  if constexpr (NPR > 0) {
    if (tid < NPR) {
      int pj = 1;
      while ((pj + 1) * pj / 2 <= tid) ++pj;
      cholesky_general_dpair<A>(Ld, pj, tid - pj * (pj - 1) / 2, c, r, Tm, anyv0, pc + tid * kBGGPc);
    }
  }
  // per-asset log2-unit coefficients, as basket_kernel
  const double dt = Tm / static_cast<double>(T);
  const double sq = sqrt(dt);
  constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
  float ca[A], x0[A], Lb[A][A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double drift = r - d - 0.5 * v * v;
    ca[i] = static_cast<float>(drift * dt * kBLog2e);
    const double bi = v * sq * kBLog2e * zscale;
    x0[i] = static_cast<float>(c[4 + i]);
#pragma unroll
    for (int k = 0; k < A; ++k) Lb[i][k] = k <= i ? static_cast<float>(bi * Ld[i * kMaxAssets + k]) : 0.0f;
  }
  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);

  // payoff constants (basket_general_kernel's), the weights and the scalar constants of the table
  const float Tf = static_cast<float>(Tm);
  const float df = math::exp_any(static_cast<float>(-r) * Tf);
  const float Kf = static_cast<float>(c[0]);
  float wt[A];  // the same for every lane: kept in scalar registers
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const float w = g.weights ? static_cast<float>(g.weights[b * g.weights_stride + i]) : static_cast<float>(1.0 / A);
    wt[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, w)));
  }
  const float cT = Tm == 0.0 ? 0.0f : static_cast<float>(1.0 / (2.0 * Tm));
  const float crho = df * (Tf * Kf);
  const float rr = static_cast<float>(r);
  auto forward = [&](int i) {
    return static_cast<float>(c[4 + i]) * math::exp_any(static_cast<float>(r - c[4 + A + i]) * Tf);
  };
  // the constants that need no sum, per asset: ix0, cv and RAW's s, av, aT (a wave the pairs above do not hold up)
  if (tid >= 64 && tid < 64 + A) {
    const int i = tid - 64;
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double mu = r - d - 0.5 * v * v;
    float* f = fc + i * kBGGFc;
    f[0] = 1.0f;
    f[1] = static_cast<float>(1.0 / c[4 + i]);
    f[2] = v == 0.0 ? 0.0f : static_cast<float>(1.0 / v);
    f[3] = v == 0.0 ? 0.0f : static_cast<float>(-mu * Tm / v - v * Tm);
    f[4] = static_cast<float>(mu / 2.0);
  }
  __syncthreads();

  auto valid_paths = [&](int64_t chunk) {  // how many of the lane's 4 values of this chunk are paths (< P)
    const int64_t left = P - chunk - kBPaths * static_cast<int64_t>(tid);
    return static_cast<int>(left <= 0 ? 0 : (left >= kBPaths ? kBPaths : left));
  };
  auto simulate = [&](int64_t chunk, float(&x)[A][kBPaths]) {
    PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
    basket_lane_paths<A, HW>(s, ca, x0, Lb, T, x);
  };
  auto load_parked = [&](int64_t chunk, float(&x)[A][kBPaths]) {  // the lane's own values: no barrier needed
#pragma unroll
    for (int i = 0; i < A; ++i) {
      const v4f q = park[(i * P4 + chunk) / kBPaths + tid];
#pragma unroll
      for (int j = 0; j < kBPaths; ++j) x[i][j] = q[j];
    }
  };
  // terminal sums of one chunk in basket_price_kernel's order
  auto add_terminal = [&](const float(&x)[A][kBPaths], int nvalid, double(&acc)[A]) {
#pragma unroll
    for (int i = 0; i < A; ++i) {
      float p = 0.0f;
#pragma unroll
      for (int j = 0; j < kBPaths; ++j) p += j < nvalid ? x[i][j] : 0.0f;
      acc[i] += static_cast<double>(p);
    }
  };
  // a lane's partials of n pass-1 sums from slot s0 on through the wave butterfly; finish_sums then adds waves 0..7
  // of tot and (with_m) of M (else 0) and reports them
  auto wave_sums = [&](const auto& acc, int s0) {
    constexpr int n = static_cast<int>(sizeof(acc) / sizeof(double));
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const double w = bwave_sum(acc[i]);
      if (lane == 0) wsum[wave * kBGGSums + s0 + i] = w;
    }
  };
  auto finish_sums = [&](bool with_m) {
    __syncthreads();
    if (tid < kBGGSums) {
      const bool is_m = tid >= kMaxAssets;
      const int p = is_m ? tid - kMaxAssets : tid;
      if (p < (is_m ? NM : A)) {
        double sum = 0.0;
        if (!is_m || with_m)
          for (int w = 0; w < kBWaves; ++w) sum += wsum[w * kBGGSums + tid];
        tot[tid] = sum;
        if (sums) sums[b * (A + NM) + (is_m ? A : 0) + p] = sum;
      }
    }
    __syncthreads();
  };
  // One pass over the paths for the sums that come before the payoffs: TOT the terminal sums (the first pass over
  // the paths: it simulates and, in the lds mode, parks), MOM the moments M_im = sum f64(x_i L_m), m <= i.  A <= 4
  // takes both together; from A = 5 on TOT goes first, alone (basket_greeks_kernel's plan).
  auto sum_pass = [&](auto tot_tag, auto mom_tag) {
    constexpr bool TOT = decltype(tot_tag)::value, MOM = decltype(mom_tag)::value;
    double acc[A], accm[NM];
#pragma unroll
    for (int i = 0; i < A; ++i) acc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NM; ++i) accm[i] = 0.0;
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float x[A][kBPaths];
        if constexpr (MODE == kBPriceLds && !TOT) load_parked(chunk, x);
        else simulate(chunk, x);
        if constexpr (TOT) add_terminal(x, nvalid, acc);
        if constexpr (MOM) {
#pragma unroll
          for (int j = 0; j < kBPaths; ++j) {
            if (j < nvalid) {
              float L[A];
#pragma unroll
              for (int i = 0; i < A; ++i) L[i] = basket_greeks_log<HW>(x[i][j], x0[i]);
#pragma unroll
              for (int i = 0; i < A; ++i)
#pragma unroll
                for (int m = 0; m <= i; ++m) accm[i * (i + 1) / 2 + m] += static_cast<double>(x[i][j] * L[m]);
            }
          }
        }
        if constexpr (MODE == kBPriceLds && TOT) {
          // slot (chunk + 4 tid) / 4 of row i: chunk + 4 tid < P, so the slot ends at or before P4
#pragma unroll
          for (int i = 0; i < A; ++i)
            park[(i * P4 + chunk) / kBPaths + tid] = v4f{x[i][0], x[i][1], x[i][2], x[i][3]};
        }
      }
    }
    if constexpr (TOT) wave_sums(acc, 0);
    if constexpr (MOM) wave_sums(accm, kMaxAssets);
  };
  constexpr bool kSplitRaw = NP > 1;  // RAW: the terminal sums ride along with a single payoff pass only
  constexpr bool kSplitMom = A > 4;
  using yes = std::true_type;
  using no = std::false_type;

  if constexpr (MODE != kBPriceRaw) {
    if constexpr (kSplitMom) {
      sum_pass(yes{}, no{});
      sum_pass(no{}, yes{});
    } else {
      sum_pass(yes{}, yes{});
    }
    finish_sums(true);
    if (tid >= 256 && tid < 256 + A) {  // the per-asset constants that move with the sums
      const int i = tid - 256;
      const double v = c[4 + 2 * A + i], rd = r - c[4 + A + i];
      const double lbar = tot[kMaxAssets + i * (i + 1) / 2 + i] / tot[i];
      float* f = fc + i * kBGGFc;
      f[0] = forward(i) / static_cast<float>(tot[i] / static_cast<double>(P));
      f[3] = v == 0.0 ? 0.0f : static_cast<float>(-lbar / v);
      f[4] = Tm == 0.0 ? static_cast<float>(rd) : static_cast<float>(-lbar / (2.0 * Tm) + rd);
    }
    if (tid < NPR * kMaxAssets) {  // ac_i^q of pair q = tid / 8, asset i = tid % 8, from the f32 g^q, g0^q the paths see
      const int q = tid >> 3, i = tid & 7;
      if (i < A) {
        float* p = pc + q * kBGGPc;
        double s = static_cast<double>(p[kMaxAssets * kMaxAssets + i]);
        for (int m = 0; m <= i; ++m)
          s = s + static_cast<double>(p[i * kMaxAssets + m]) * (tot[kMaxAssets + i * (i + 1) / 2 + m] / tot[i]);
        p[kMaxAssets * kMaxAssets + kMaxAssets + i] = static_cast<float>(-s);
      }
    }
    __syncthreads();
  } else if constexpr (kSplitRaw) {  // RAW with several payoff passes: the terminal sums in a pass of their own
    sum_pass(yes{}, no{});
    finish_sums(false);
  }

  // one path's terms of pass PASS (the table of the header), each cast to f64 and added with its square
  double v[2 * TP];
  auto payoffs = [&](auto tag, const float(&x)[A][kBPaths], int nvalid) {
    constexpr int T0 = decltype(tag)::value * TP;
    constexpr int T1 = T0 + TP < NT ? T0 + TP : NT;
    constexpr bool kTheta = T0 <= 4 * A + 3 && T1 > 4 * A + 2;
#pragma unroll
    for (int j = 0; j < kBPaths; ++j) {
      if (j < nvalid) {
        // from A = 4 on the LDS constants are read again for every path, not held across the path loop
        if constexpr (A > 3) asm volatile("" ::: "memory");
        float L[A], w[A];
        float bk = 0.0f;
#pragma unroll
        for (int i = 0; i < A; ++i) {
          const float xs = x[i][j] * fc[i * kBGGFc];
          bk = bk + wt[i] * xs;
          w[i] = (df * xs) * wt[i];
          L[i] = basket_greeks_log<HW>(x[i][j], x0[i]);
        }
        const float dp = Kf - bk, dc = bk - Kf;
        const bool ip = dp > 0.0f, ic = dc > 0.0f;
        const float put = df * (ip ? dp : 0.0f), call = df * (ic ? dc : 0.0f);
        float sT = 0.0f;
        if constexpr (kTheta) {
#pragma unroll
          for (int i = 0; i < A; ++i) sT = sT + w[i] * (L[i] * cT + fc[i * kBGGFc + 4]);
        }
        // sC^q = ((0 + w_j hc_j) + w_{j+1} hc_{j+1}) + ..., hc_i = c_i^q + ac_i^q, rows i >= j of pair q = (j, k)
        auto pair_sum = [&](auto qtag) {
          constexpr int q = decltype(qtag)::value;
          constexpr int pj = basket_ggreek_pair_row(q);
          const float* p = pc + q * kBGGPc;
          float sC = 0.0f;
#pragma unroll
          for (int i = pj; i < A; ++i) {
            float ci = p[kMaxAssets * kMaxAssets + i];
#pragma unroll
            for (int m = 0; m <= i; ++m) ci = ci + p[i * kMaxAssets + m] * L[m];
            sC = sC + w[i] * (ci + p[kMaxAssets * kMaxAssets + kMaxAssets + i]);
          }
          return sC;
        };
        basket_static_for(std::make_integer_sequence<int, T1 - T0>{}, [&](auto ktag) {
          constexpr int k = decltype(ktag)::value;
          constexpr int term = T0 + k;
          float t;
          if constexpr (term < 4 * A) {
            constexpr int kind = term / A, i = term % A;  // 0 delta put, 1 delta call, 2 vega put, 3 vega call
            const float* f = fc + i * kBGGFc;
            const float wx = kind < 2 ? w[i] * f[1] : w[i] * (L[i] * f[2] + f[3]);
            t = (kind & 1) ? (ic ? wx : 0.0f) : (ip ? -wx : 0.0f);
          } else if constexpr (term == 4 * A) {
            t = ip ? -crho : 0.0f;
          } else if constexpr (term == 4 * A + 1) {
            t = ic ? crho : 0.0f;
          } else if constexpr (term == 4 * A + 2) {
            t = rr * put + (ip ? sT : 0.0f);
          } else if constexpr (term == 4 * A + 3) {
            t = rr * call - (ic ? sT : 0.0f);
          } else if constexpr (term < NG) {
            const float sC = pair_sum(std::integral_constant<int, (term - PT0) / 2>{});
            t = ((term - PT0) & 1) ? (ic ? sC : 0.0f) : (ip ? -sC : 0.0f);
          } else {
            t = term == NG ? put : call;
          }
          const double d = static_cast<double>(t);
          v[k] += d;
          v[TP + k] += d * d;
        });
      }
    }
  };

  const double n = static_cast<double>(P);
  double* out = greeks + b * (2 * NG + 4);
#pragma unroll 1
  for (int pass = 0; pass < NP; ++pass) {
#pragma unroll
    for (int k = 0; k < 2 * TP; ++k) v[k] = 0.0;
    double acc[A];  // RAW with one payoff pass: the terminal sums ride along
#pragma unroll
    for (int i = 0; i < A; ++i) acc[i] = 0.0;
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float x[A][kBPaths];
        if constexpr (MODE == kBPriceLds) load_parked(chunk, x);
        else simulate(chunk, x);
        if constexpr (MODE == kBPriceRaw && !kSplitRaw) add_terminal(x, nvalid, acc);
        basket_static_for(std::make_integer_sequence<int, NP>{}, [&](auto tag) {
          if (NP == 1 || pass == decltype(tag)::value) payoffs(tag, x, nvalid);
        });
      }
    }
    if constexpr (MODE == kBPriceRaw && !kSplitRaw) {
      wave_sums(acc, 0);
      finish_sums(false);  // M = 0
    }
    // the pass's sums: wave butterfly, waves 0..7, sum k totalled by thread k
#pragma unroll
    for (int k = 0; k < 2 * TP; ++k) {
      const double w = bwave_sum(v[k]);
      if (lane == 0) lds[wave * kBGGRed + k] = w;
    }
    __syncthreads();
    const int term = pass * TP + tid;
    if (tid < TP && term < NT) {  // a term's mean and standard error
      auto total = [&](int k) {
        double t2 = 0.0;
        for (int w = 0; w < kBWaves; ++w) t2 += lds[w * kBGGRed + k];
        return t2;
      };
      double m = total(tid) / n;
      double se = 0.0;
      if (P > 1) {
        const double var = total(TP + tid) - n * m * m;
        se = sqrt((var > 0.0 ? var : 0.0) / (n - 1.0) / n);
      }
      if (term < PT0) {
        out[term] = m;
        out[NG + term] = se;
      } else if (term < NG) {  // pair q, put at 4A + 4 + q, call at 4A + 4 + np + q
        if (anyv0) m = se = __builtin_nan("");
        const int col = PT0 + ((term - PT0) & 1) * NPR + ((term - PT0) >> 1);
        out[col] = m;
        out[NG + col] = se;
      } else {  // the prices: columns 2n, 2n + 1 and 2n + 2, 2n + 3
        out[NG + term] = m;
        out[NG + term + 2] = se;
      }
    }
    if (NP > 1) __syncthreads();  // the partials are rewritten by the next pass
  }
}

// ---- Greeks of the Asian and lookback basket options: basket_path_greeks_kernel (smc_basket_greeks_paths) ----
// basket_path_kernel's front end, row hook and sweeps of whole dates (restated, not shared: its registers stay as
// they are) with path_greeks_kernel's per-row log-derivative tables, asset by asset: asset i's volatility and spot
// move only its own rows, so with L_it = log(x_it / X0_i) the row tables av_it, aT_it, tau_t and s_it give
// d ln xs_it / dv_i = L_it cv_i + av_it, / dT = L_it cT + aT_it, / dr = tau_t, / dX0_i = 1 / X0_i (the table of
// include/spectralmc_hip.h).  8A + 12 per-path f32 terms, each cast to f64 and added with its square.
//   tables     [T][3A + 1] f32 in LDS in both normalisations: s_it, av_it, aT_it per asset, then tau_t.
//   NORMALIZE  first the 2 A T row sums (x and x L per asset and row) as per-lane f64 accumulators in dynamic LDS
//              ([dates * 2A][512], lane tid touches column tid only) in sweeps of whole dates, each re-simulating
//              from row 0; the thread that totals an (asset, row) pair writes its three table entries.
// Passes (basket_pg_pass): a payoff simulation takes at most 22 terms.  A <= 4: {Asian, all assets, rho, theta,
// price}, {lookback put and call, all of theirs}.  A = 5..8, passes of at most 16 terms: Asian {rho, theta, price},
// then the assets in ranges of 4 (A = 5, 6: {0..3}, {4..A-1}) or of 2 (A = 7, 8: {0, 1}, {2, 3}, {4, 5}, {6..A-1});
// lookback put {deltas, rho, theta, price}, {vegas}; lookback call likewise: 7 passes for A = 5, 6 and 9 for A = 7, 8.
// A lookback pass keeps the A raw values of the extreme row and takes their logs after the rows.  A sum belongs to
// one pass and keeps its order, so no value depends on the plan.
struct BasketPGPass {
  bool asian, lmin, lmax;
  bool scal;  // Asian: rho, theta and the price ride along; lookback: the deltas, rho, theta and the price are taken
  bool vega;  // lookback: the vegas are taken
  int a0, a1;  // Asian: the assets whose delta and vega the pass takes
};
constexpr int basket_pg_range(int A) { return A <= 6 ? 4 : 2; }  // assets per Asian delta / vega pass (A >= 5)
constexpr int basket_pg_ranges(int A) { return (A + basket_pg_range(A) - 1) / basket_pg_range(A); }
constexpr int basket_pg_passes(int A) { return A <= 4 ? 2 : 5 + basket_pg_ranges(A); }
constexpr BasketPGPass basket_pg_pass(int A, int p) {
  if (A <= 4)
    return p == 0 ? BasketPGPass{true, false, false, true, false, 0, A}
                  : BasketPGPass{false, true, true, true, true, 0, A};
  const int nr = basket_pg_ranges(A), rs = basket_pg_range(A);
  if (p == 0) return BasketPGPass{true, false, false, true, false, 0, 0};
  if (p <= nr) return BasketPGPass{true, false, false, false, false, (p - 1) * rs, p * rs < A ? p * rs : A};
  return p == nr + 1   ? BasketPGPass{false, true, false, true, false, 0, A}
         : p == nr + 2 ? BasketPGPass{false, true, false, false, true, 0, A}
         : p == nr + 3 ? BasketPGPass{false, false, true, true, false, 0, A}
                       : BasketPGPass{false, false, true, false, true, 0, A};
}
constexpr int basket_pg_extreme_terms(BasketPGPass p, int A) { return (p.scal ? A + 3 : 0) + (p.vega ? A : 0); }
constexpr int basket_pg_terms(BasketPGPass p, int A) {
  return p.asian ? 4 * (p.a1 - p.a0) + (p.scal ? 6 : 0)
                 : ((p.lmin ? 1 : 0) + (p.lmax ? 1 : 0)) * basket_pg_extreme_terms(p, A);
}
constexpr int kBPGMaxTerms = 22;
// scratch at the head of the dynamic LDS: pass partials [kBWaves][2 kBPGMaxTerms] and the Cholesky factor [8][8]
// (f64; 3328 B)
constexpr int kBPGHead = kBWaves * 2 * kBPGMaxTerms + kMaxAssets * kMaxAssets;
constexpr size_t kBPGScratch = kBPGHead * sizeof(double);
static_assert(kBPGScratch == 3328 && kBPGScratch % 16 == 0, "the header states the scratch bytes");

template <int A, bool HW, bool NORMALIZE>
__global__ __launch_bounds__(kBThreads) void basket_path_greeks_kernel(BasketArgs a, BasketGeneralArgs g,
                                                                       double* __restrict__ greeks, int sweep_dates) {
  constexpr int NP = basket_pg_passes(A);
  constexpr int REC = 3 * A + 1;   // a row's table record: s [A], av [A], aT [A], tau
  constexpr int NG = 2 * A + 2;    // Greek kinds
  constexpr int RED = 2 * kBPGMaxTerms;
  // kBPGHead doubles of scratch; the tables ([T][REC] f32, padded to 8 B); NORMALIZE: the accumulator rows
  // ([sweep_dates * 2A][512])
  extern __shared__ double lds[];
  double* Ld = lds + kBWaves * RED;  // [8][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int T = a.T;
  const int64_t P = a.P;
  float* tab = reinterpret_cast<float*>(lds + kBPGHead);
  double* acc = lds + kBPGHead + (static_cast<size_t>(REC) * T * sizeof(float) + 7) / 8;

  const double* c = a.contracts + b * (3 * A + 4);
  const double Tm = c[1], r = c[2], rho = c[3];
  if (tid == 0) cholesky_general(A, rho, g.corr ? g.corr + b * g.corr_stride : nullptr, Ld);
  __syncthreads();
  // per-asset log2-unit coefficients, as basket_kernel
  const double dt = Tm / static_cast<double>(T);
  const double sq = sqrt(dt);
  constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
  float ca[A], x0[A], Lb[A][A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i], d = c[4 + A + i];
    const double drift = r - d - 0.5 * v * v;
    ca[i] = static_cast<float>(drift * dt * kBLog2e);
    const double bi = v * sq * kBLog2e * zscale;
    x0[i] = static_cast<float>(c[4 + i]);
#pragma unroll
    for (int k = 0; k < A; ++k) Lb[i][k] = k <= i ? static_cast<float>(bi * Ld[i * kMaxAssets + k]) : 0.0f;
  }
  const uint64_t ordinal = static_cast<uint64_t>((a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0 + b);

  auto uniform = [](float f) {  // the same for every lane: kept in a scalar register
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, f)));
  };
  auto valid_paths = [&](int64_t chunk) {  // how many of the lane's 4 values of this chunk are paths (< P)
    const int64_t left = P - chunk - kBPaths * static_cast<int64_t>(tid);
    return static_cast<int>(left <= 0 ? 0 : (left >= kBPaths ? kBPaths : left));
  };
  // Row t's table entries of asset i from the f64 contract row (and, under NORMALIZE, the pair's two sums)
  auto write_entry = [&](int t, int i, double sumx, double sumxl) {
    const double v = c[4 + 2 * A + i], rd = r - c[4 + A + i];
    const double mu = rd - 0.5 * v * v;
    const double tau = t == T - 1 ? Tm : static_cast<double>(t + 1) * dt;
    const double fr = static_cast<double>(t + 1) / static_cast<double>(T);
    float* rec = tab + static_cast<size_t>(t) * REC;
    if (i == 0) rec[3 * A] = static_cast<float>(tau);
    if constexpr (NORMALIZE) {
      const float F = static_cast<float>(c[4 + i]) * math::exp_any(static_cast<float>(rd) * static_cast<float>(tau));
      const double lbar = sumxl / sumx;
      rec[i] = F / static_cast<float>(sumx / static_cast<double>(P));
      rec[A + i] = v == 0.0 ? 0.0f : static_cast<float>(-lbar / v);
      rec[2 * A + i] = Tm == 0.0 ? static_cast<float>(rd * fr) : static_cast<float>(-lbar / (2.0 * Tm) + rd * fr);
    } else {
      rec[i] = 1.0f;
      rec[A + i] = v == 0.0 ? 0.0f : static_cast<float>(-mu * tau / v - v * tau);
      rec[2 * A + i] = static_cast<float>(mu / 2.0 * fr);
    }
  };

  if constexpr (NORMALIZE) {
    for (int t0 = 0; t0 < T; t0 += sweep_dates) {
      const int nd = T - t0 < sweep_dates ? T - t0 : sweep_dates;
      const int nrows = 2 * nd * A;  // <= the rows the host sized acc for; row 2 (d A + i): x, the next one: x L
      for (int q = 0; q < nrows; ++q) acc[q * kBThreads + tid] = 0.0;
      for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
        const int nvalid = valid_paths(chunk);
        if (nvalid > 0) {
          PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
          float x[A][kBPaths];
          basket_lane_paths<A, HW>(s, ca, x0, Lb, t0 + nd, x, [&](const float(&xr)[A][kBPaths], int t) {
            if (t >= t0) {  // t < t0 + nd: date t - t0 of this sweep, the lane's own column
              double* row = acc + static_cast<size_t>(t - t0) * 2 * A * kBThreads + tid;
#pragma unroll
              for (int i = 0; i < A; ++i) {
                float p = 0.0f;  // basket_path_kernel's row sum: the valid values left to right in f32 from 0
#pragma unroll
                for (int j = 0; j < kBPaths; ++j) p += j < nvalid ? xr[i][j] : 0.0f;
                row[(2 * i) * kBThreads] += static_cast<double>(p);
                double sl = row[(2 * i + 1) * kBThreads];
#pragma unroll
                for (int j = 0; j < kBPaths; ++j)
                  if (j < nvalid) sl += static_cast<double>(xr[i][j] * basket_greeks_log<HW>(xr[i][j], x0[i]));
                row[(2 * i + 1) * kBThreads] = sl;
              }
            }
          });
        }
      }
      for (int q = 0; q < nrows; ++q) {  // wave butterfly into lane 0's own slot
        const double w = bwave_sum(acc[q * kBThreads + tid]);
        if (lane == 0) acc[q * kBThreads + tid] = w;
      }
      __syncthreads();
      if (tid < nd * A) {  // pair tid = d A + i: waves 0..7 of its two sums, then its table entries
        double sumx = 0.0, sumxl = 0.0;
        for (int w = 0; w < kBWaves; ++w) sumx += acc[(2 * tid) * kBThreads + w * 64];
        for (int w = 0; w < kBWaves; ++w) sumxl += acc[(2 * tid + 1) * kBThreads + w * 64];
        const int d = tid / A;
        write_entry(t0 + d, tid - d * A, sumx, sumxl);
      }
      __syncthreads();  // the accumulators are free for the next sweep
    }
  } else {
    for (int idx = tid; idx < A * T; idx += kBThreads) {
      const int t = idx / A;
      write_entry(t, idx - t * A, 0.0, 0.0);
    }
    __syncthreads();
  }

  // payoff constants (basket_path_kernel's), the weights and the per-asset constants of the table
  const float Tf = static_cast<float>(Tm);
  const float df = math::exp_any(static_cast<float>(-r) * Tf);
  const float Kf = static_cast<float>(c[0]);
  const float steps = static_cast<float>(T);
  const float cT = Tm == 0.0 ? 0.0f : static_cast<float>(1.0 / (2.0 * Tm));
  const float rr = static_cast<float>(r);
  float wt[A], ix0[A], cv[A];
#pragma unroll
  for (int i = 0; i < A; ++i) {
    const double v = c[4 + 2 * A + i];
    wt[i] = uniform(g.weights ? static_cast<float>(g.weights[b * g.weights_stride + i]) : static_cast<float>(1.0 / A));
    ix0[i] = uniform(static_cast<float>(1.0 / c[4 + i]));
    cv[i] = uniform(v == 0.0 ? 0.0f : static_cast<float>(1.0 / v));
  }
  const float inf = __builtin_huge_valf();
  const double n = static_cast<double>(P);
  double* out = greeks + b * (8 * NG + 8);

  basket_static_for(std::make_integer_sequence<int, NP>{}, [&](auto tag) {
    constexpr BasketPGPass PS = basket_pg_pass(A, decltype(tag)::value);
    constexpr int NTP = basket_pg_terms(PS, A);
    constexpr bool ASIAN = PS.asian, LMIN = PS.lmin, LMAX = PS.lmax, SCAL = PS.scal, VEGA = PS.vega;
    constexpr int A0 = PS.a0, A1 = PS.a1, NR = A1 - A0 > 0 ? A1 - A0 : 1;
    constexpr int NE = basket_pg_extreme_terms(PS, A);  // a lookback payoff's terms in this pass
    constexpr int V0 = SCAL ? A : 0;                    // the first vega among them (after the deltas)
    constexpr int S0 = VEGA ? 2 * A : A;                // rho, theta, price (after the deltas and the vegas)
    static_assert(NTP <= kBPGMaxTerms, "pass partials");
    double v[2 * NTP];  // term k of the pass: v[k], its squares: v[NTP + k]
#pragma unroll
    for (int k = 0; k < 2 * NTP; ++k) v[k] = 0.0;
    auto add = [&](int k, float t) {
      const double d = static_cast<double>(t);
      v[k] += d;
      v[NTP + k] += d * d;
    };
    // a lookback payoff's terms (delta_i, then vega_i, then rho, theta, price: those the pass takes) from its extreme
    // u, the extreme's row te and the A raw values there
    auto extreme_terms = [&](bool is_put, float u, int te, const float(&xe)[A][kBPaths], int j, int base) {
      const float* rec = tab + static_cast<size_t>(te) * REC;  // te < T: every valid path has T >= 1 rows
      const float diff = is_put ? Kf - u : u - Kf;
      const bool in = diff > 0.0f;
      const float pay = df * (in ? diff : 0.0f);
      float gT = 0.0f;
#pragma unroll
      for (int i = 0; i < A; ++i) {
        const float xs = NORMALIZE ? xe[i][j] * rec[i] : xe[i][j];
        const float wx = wt[i] * xs;
        const float L = basket_greeks_log<HW>(xe[i][j], x0[i]);
        const float wd = (df * wx) * ix0[i];
        const float wv = df * (wx * (L * cv[i] + rec[A + i]));
        gT = gT + wx * (L * cT + rec[2 * A + i]);
        if constexpr (SCAL) add(base + i, in ? (is_put ? -wd : wd) : 0.0f);
        if constexpr (VEGA) add(base + V0 + i, in ? (is_put ? -wv : wv) : 0.0f);
      }
      if constexpr (SCAL) {
        const float wr = df * (u * rec[3 * A]), wT = df * gT;
        add(base + S0, is_put ? -(Tf * pay) - (in ? wr : 0.0f) : -(Tf * pay) + (in ? wr : 0.0f));
        add(base + S0 + 1, is_put ? rr * pay + (in ? wT : 0.0f) : rr * pay - (in ? wT : 0.0f));
        add(base + S0 + 2, pay);
      }
    };
    for (int64_t chunk = 0; chunk < P; chunk += kBChunk) {
      const int nvalid = valid_paths(chunk);
      if (nvalid > 0) {
        float sa[kBPaths], sT[kBPaths], sr[kBPaths], sd[NR][kBPaths], sv[NR][kBPaths];
        float mn[kBPaths], mx[kBPaths], xmn[A][kBPaths], xmx[A][kBPaths];
        int tmn[kBPaths], tmx[kBPaths];
#pragma unroll
        for (int j = 0; j < kBPaths; ++j) {
          sa[j] = sT[j] = sr[j] = 0.0f;
          mn[j] = inf;
          mx[j] = -inf;
          tmn[j] = tmx[j] = 0;
#pragma unroll
          for (int i = 0; i < A1 - A0; ++i) sd[i][j] = sv[i][j] = 0.0f;
#pragma unroll
          for (int i = 0; i < A; ++i) xmn[i][j] = xmx[i][j] = x0[i];
        }
        PathStream s(a.seed, ordinal, static_cast<uint64_t>(chunk / kBPaths + tid));
        float x[A][kBPaths];
        basket_lane_paths<A, HW>(s, ca, x0, Lb, T, x, [&](const float(&xr)[A][kBPaths], int t) {
          const float* rec = tab + static_cast<size_t>(t) * REC;
#pragma unroll
          for (int j = 0; j < kBPaths; ++j) {
            float wx[A];
            float bt = 0.0f;
#pragma unroll
            for (int i = 0; i < A; ++i) {
              const float xs = NORMALIZE ? xr[i][j] * rec[i] : xr[i][j];
              wx[i] = wt[i] * xs;
              bt = bt + wx[i];
            }
            if constexpr (ASIAN) {
              sa[j] = sa[j] + bt;
              float L[A];
#pragma unroll
              for (int i = 0; i < A; ++i)
                if (SCAL || (i >= A0 && i < A1)) L[i] = basket_greeks_log<HW>(xr[i][j], x0[i]);
#pragma unroll
              for (int i = A0; i < A1; ++i) {
                sd[i - A0][j] = sd[i - A0][j] + wx[i];
                sv[i - A0][j] = sv[i - A0][j] + wx[i] * (L[i] * cv[i] + rec[A + i]);
              }
              if constexpr (SCAL) {
                float rowT = 0.0f;
#pragma unroll
                for (int i = 0; i < A; ++i) rowT = rowT + wx[i] * (L[i] * cT + rec[2 * A + i]);
                sT[j] = sT[j] + rowT;
                sr[j] = sr[j] + bt * rec[3 * A];
              }
            }
            if constexpr (LMIN) {
              if (bt < mn[j]) {  // strict: the first row wins a tie
                mn[j] = bt;
                tmn[j] = t;
#pragma unroll
                for (int i = 0; i < A; ++i) xmn[i][j] = xr[i][j];
              }
            }
            if constexpr (LMAX) {
              if (bt > mx[j]) {
                mx[j] = bt;
                tmx[j] = t;
#pragma unroll
                for (int i = 0; i < A; ++i) xmx[i][j] = xr[i][j];
              }
            }
          }
        });
#pragma unroll
        for (int j = 0; j < kBPaths; ++j) {
          if (j < nvalid) {
            if constexpr (ASIAN) {
              const float avg = sa[j] / steps;
              const float dp = Kf - avg, dc = avg - Kf;
              const bool ip = dp > 0.0f, ic = dc > 0.0f;
              const float put = df * (ip ? dp : 0.0f), call = df * (ic ? dc : 0.0f);
#pragma unroll
              for (int i = 0; i < A1 - A0; ++i) {
                const float wd = df * ((sd[i][j] / steps) * ix0[A0 + i]);
                const float wv = df * (sv[i][j] / steps);
                add(4 * i, ip ? -wd : 0.0f);
                add(4 * i + 1, ic ? wd : 0.0f);
                add(4 * i + 2, ip ? -wv : 0.0f);
                add(4 * i + 3, ic ? wv : 0.0f);
              }
              if constexpr (SCAL) {
                const float wr = df * (sr[j] / steps), wT = df * (sT[j] / steps);
                add(4 * (A1 - A0), -(Tf * put) - (ip ? wr : 0.0f));
                add(4 * (A1 - A0) + 1, -(Tf * call) + (ic ? wr : 0.0f));
                add(4 * (A1 - A0) + 2, rr * put + (ip ? wT : 0.0f));
                add(4 * (A1 - A0) + 3, rr * call - (ic ? wT : 0.0f));
                add(4 * (A1 - A0) + 4, put);
                add(4 * (A1 - A0) + 5, call);
              }
            }
            if constexpr (LMIN) extreme_terms(true, mn[j], tmn[j], xmn, j, 0);
            if constexpr (LMAX) extreme_terms(false, mx[j], tmx[j], xmx, j, LMIN ? NE : 0);
          }
        }
      }
    }
    // the pass's sums: wave butterfly, waves 0..7, sum k totalled by thread k alone
#pragma unroll
    for (int k = 0; k < 2 * NTP; ++k) {
      const double w = bwave_sum(v[k]);
      if (lane == 0) lds[wave * RED + k] = w;
    }
    __syncthreads();
    if (tid < NTP) {  // a term's mean and standard error, and its column: Greek kind gk of payoff q, or price q
      auto total = [&](int k) {
        double t2 = 0.0;
        for (int w = 0; w < kBWaves; ++w) t2 += lds[w * RED + k];
        return t2;
      };
      const double m = total(tid) / n;
      double se = 0.0;
      if (P > 1) {
        const double var = total(NTP + tid) - n * m * m;
        se = sqrt((var > 0.0 ? var : 0.0) / (n - 1.0) / n);
      }
      int gk, q;
      if constexpr (ASIAN) {
        if (tid < 4 * (A1 - A0)) {
          const int i = A0 + (tid >> 2), sub = tid & 3;
          gk = sub < 2 ? i : A + i;
          q = sub & 1;
        } else {
          const int kk = tid - 4 * (A1 - A0);  // rho put, rho call, theta put, theta call, put, call
          gk = 2 * A + (kk >> 1);
          q = kk & 1;
        }
      } else {
        const int e = tid / NE, kk = tid - e * NE;  // delta_i, vega_i, rho, theta, price: those the pass takes
        gk = SCAL ? (VEGA || kk < A ? kk : A + kk) : A + kk;
        q = LMIN ? 2 + e : 3;
      }
      if (gk < NG) {
        out[4 * gk + q] = m;
        out[4 * NG + 4 * gk + q] = se;
      } else {
        out[8 * NG + q] = m;
        out[8 * NG + 4 + q] = se;
      }
    }
    if (NP > 1) __syncthreads();  // the partials are rewritten by the next pass
  });
}


// ---- basket_resident_kernel: the terminal rows never leave the chip ------------------------------
// A C5 contract's terminal rows are A x P f32 = 2 MiB, far beyond one CU, so W = P / 4096
// co-resident workgroups run it (slice s = paths [4096 s, 4096 (s + 1)) = batch rows
// [s M/W, (s+1) M/W)), one 4096-path chunk each: lane l advances paths 4096 s + 4 l .. + 3 of all A
// assets through the 16 rows (one dwordx4 buffer store per asset and row) and keeps their terminal
// values.  The payoff needs every slice's terminal sums (the per-asset forward scales), so the
// exchange is pipelined one contract deep.  Iteration j of a workgroup:
//   0. wave 0 polls for contract j - 1's slice sums (published by every partner at the end of its
//      iteration j - 1), gathers them in one round of loads and writes the per-asset scales to LDS,
//      while waves 1..15 already simulate;
//   1. all waves simulate contract j (coefficients from an LDS table that wave 0 fills for 64
//      contracts at a time, one contract per lane: the f64 Cholesky is off the per-contract path);
//   2. the basket put of contract j - 1 from the terminal values parked in LDS (one 16-B slot per
//      lane and asset), column sums over the slice's rows (groups in order) stored to the launch's
//      column buffer [B][W][N]; contract j's terminal values replace j - 1's in the slots;
//   3. wave 0 publishes contract j's slice sums (write-through stores, one drain, an arrival add)
//      while the other waves move on.
// basket_mean_fft_kernel then adds each contract's W column sums in slice order, takes the M-mean
// and runs the FFT.  Only wave 0 ever waits on global memory.  Slice-sum slots rotate over 4
// contracts: a workgroup writes contract j's slots after its wait in iteration j saw every partner
// finish iteration j - 1, long after their reads of contract j - 4.  Reduction orders:
// oracle_basket_kernel(wg = 1024, slices = W).
constexpr int kRThreads = 1024;
constexpr int kRWaves = kRThreads / 64;
constexpr int kRChunk = kRThreads * kBPaths;  // 4096 paths: one chunk per workgroup and contract
constexpr int kRMaxSlices = 32;
constexpr int kRowBlock = 16;
constexpr int kRSlots = 4;                   // slice-sum slots (contract j mod 4)
constexpr int kRTable = 64;                  // contracts per coefficient table (one per wave-0 lane)

// Sync area of the resident basket launch (bytes): [0, 128) done counter (+0), the sticky status
// word (+SMC_SYNC_STATUS_OFFSET), the launch's failure flag (+SMC_SYNC_LAUNCH_FAIL_OFFSET) and contract
// queue (+64); per group a 128-B line of slice-sum arrivals; slice sums [groups][4][W A + 1] f64 (the
// last entry: the contract of the group's iteration j + 2, dynamic tail); column sums [chunk][W][N].
struct BasketSyncLayout {
  int64_t groups, xsum_off, xcol_off, bytes;
};
BasketSyncLayout basket_sync_layout(int A, int W, int N, int64_t groups, int64_t chunk) {
  BasketSyncLayout l{};
  l.groups = groups;
  l.xsum_off = 128 + 128 * groups;
  l.xcol_off = (l.xsum_off + groups * kRSlots * (W * A + 1) * 8 + 255) / 256 * 256;
  l.bytes = l.xcol_off + chunk * W * static_cast<int64_t>(N) * 8;
  return l;
}

constexpr int coef_stride(int A) { return 2 * A + A * A; }  // ca[A], x0[A], Lb[A][A] (f32)

size_t basket_resident_lds_bytes(int A, int N) {
  // terminal slots [A][1024] v4f, part [4096] f64, wsum [16][A] f64, scales + contract ring, two
  // coefficient tables [64][2A + A^2] f32 and two coefficient slots of dynamic contracts
  return static_cast<size_t>(A) * kRThreads * 16 +
         (4096 + kRWaves * kMaxAssets + 16) * sizeof(double) +
         (2 * kRTable + 2) * static_cast<size_t>(coef_stride(A)) * sizeof(float);
}

struct BasketResArgs {
  BasketArgs a;
  int32_t W;              // workgroups per contract
  int32_t groups;         // contract sequences (grid = groups * W)
  uint8_t* sync;          // basket_sync_layout
  int64_t xsum_off, xcol_off;
  uint32_t spin_limit;    // polls of an exchange before it gives up (status word, NaN targets)
  int32_t withhold;       // smc_test_exchange_fault: slice W-1 of group 0 skips its first arrival
};

template <int A, bool HW, bool STORE_ALL>
__global__ __launch_bounds__(kRThreads) void basket_resident_kernel(BasketResArgs ra) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  constexpr int CS = coef_stride(A);
  extern __shared__ double lds[];
  const BasketArgs& a = ra.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, W = ra.W, groups = ra.groups;
  const int64_t P = a.P;
  // group (contract sequence) and slice of this workgroup: blocks b, b + 8, ... share an XCD
  int grp, slc;
  if (gridDim.x % (8 * W) == 0) {
    slc = static_cast<int>((blockIdx.x >> 3) % W);
    grp = static_cast<int>((blockIdx.x & 7) + 8 * (blockIdx.x / (8 * W)));
  } else {
    slc = static_cast<int>(blockIdx.x % W);
    grp = static_cast<int>(blockIdx.x / W);
  }
  v4f* term = reinterpret_cast<v4f*>(lds);                                   // [A][kRThreads]
  double* part = lds + static_cast<size_t>(A) * kRThreads * 2;               // [G][N] = [4096]
  double* wsum = part + 4096;                                                 // [kRWaves][A]
  float* pco = reinterpret_cast<float*>(wsum + kRWaves * kMaxAssets);         // scales[A], df, K
  int64_t* bidx = reinterpret_cast<int64_t*>(wsum + kRWaves * kMaxAssets + 12);  // [4] contract of iteration j
  float* table = reinterpret_cast<float*>(wsum + kRWaves * kMaxAssets + 16);  // [2][kRTable][CS]
  float* dco = table + 2 * kRTable * CS;                                      // [2][CS] dynamic contracts
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ra.sync + 128 + 128 * static_cast<int64_t>(grp));
  const int XS = W * A + 1;                // slice-sum slot: W x A sums + the group's contract of j + 2
  double* xsum = reinterpret_cast<double*>(ra.sync + ra.xsum_off) + static_cast<int64_t>(grp) * kRSlots * XS;
  double* xcol = reinterpret_cast<double*>(ra.sync + ra.xcol_off);           // [chunk][W][N]
  const int cols = N / 4;
  const int G = kRChunk / N;               // batch rows per slice
  const int q = tid % cols, g = tid / cols;
  const int64_t rows = STORE_ALL ? kRowBlock : 1;
  const int32_t pitch_b = static_cast<int32_t>(a.pitch * sizeof(float));  // A * rows * pitch_b < 2^31 (host check)
  const uint32_t lane_off = static_cast<uint32_t>(kBPaths * sizeof(float)) * tid;
  const int64_t ord0 = (a.ordinal_dev ? *a.ordinal_dev : 0) + a.ordinal0;
  const int width = 3 * A + 4;
  // contracts: grp + j groups for the first S iterations (every group has them), then the rest of
  // the launch from the queue, so groups on XCDs with more write bandwidth take more (per-XCD
  // finish times differed by up to 15 % with a static split).  Slice 0 takes the contract of
  // iteration j + 2 while publishing iteration j's slice sums; the partners read it with those sums
  // in iteration j + 1 (no added wait).
  constexpr int64_t kStaticQuarters = 3;  // statically assigned share of the iterations, in quarters
  const int64_t S = (a.B / groups) * kStaticQuarters / 4;
  const bool dyn = S >= 2;
  const int64_t n_static = dyn ? S * groups : a.B;
  uint32_t* queue = reinterpret_cast<uint32_t*>(ra.sync + 64);
  uint32_t* status = reinterpret_cast<uint32_t*>(ra.sync + SMC_SYNC_STATUS_OFFSET);
  uint32_t* launch_fail = reinterpret_cast<uint32_t*>(ra.sync + SMC_SYNC_LAUNCH_FAIL_OFFSET);
  auto bof = [&](int64_t jj) -> int64_t { return !dyn || jj < S ? grp + jj * groups : bidx[jj & 3]; };
  auto coefs = [&](int64_t bb, float* e) {  // simulation coefficients of contract bb (f64 Cholesky, rounded once)
    const double* c = a.contracts + bb * width;
    double L[kMaxAssets * kMaxAssets];
    cholesky_equicorr(A, c[3], L);
    const double dt = c[1] / static_cast<double>(kRowBlock);
    const double sq = sqrt(dt);
    constexpr double zscale = HW ? PathStream::kNormalScale<true> : 1.0;
#pragma unroll
    for (int i = 0; i < A; ++i) {
      const double v = c[4 + 2 * A + i], d = c[4 + A + i];
      const double drift = c[2] - d - 0.5 * v * v;
      e[i] = static_cast<float>(drift * dt * kBLog2e);
      e[A + i] = static_cast<float>(c[4 + i]);
      const double bi = v * sq * kBLog2e * zscale;
#pragma unroll
      for (int k = 0; k < A; ++k) e[2 * A + i * A + k] = k <= i ? static_cast<float>(bi * L[i * kMaxAssets + k]) : 0.0f;
    }
  };

  // step 0 (wave 0): the payoff constants of contract jj from every slice's terminal sums
  auto gather = [&](int64_t jj) {
    const int64_t b = bof(jj);
    const double* c = a.contracts + b * width;
    const double* xs = xsum + (jj % kRSlots) * XS;
    const uint32_t want = static_cast<uint32_t>(W) * static_cast<uint32_t>(jj + 1);
    // bounded poll; once any exchange of this launch has failed (its flag set) the others stop
    // waiting at once, so a failed launch still drains in about one poll budget
    uint32_t spins = 0;
    bool ok;
    while (!(ok = get_sc1(cnt) >= want) && get_sc1(launch_fail) == 0u && ++spins < ra.spin_limit)
      __builtin_amdgcn_s_sleep(2);
    if (!ok && lane == 0) {
      __hip_atomic_fetch_or(status, SMC_SYNC_EXCHANGE_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(launch_fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the W x A slice sums in one round of loads across the wave (<= 4 per lane), parked in part[]
    // (free until the payoff), then lanes 0..A-1 add their asset's W sums in slice order
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const __amdgpu_buffer_rsrc_t r = row_rsrc(xs);
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = lane + 64 * k < W * A ? lane + 64 * k : 0;
      v[k] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, idx * 8, 0, 16 /* sc1 */));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (lane + 64 * k < W * A) part[lane + 64 * k] = v[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    if (lane < A) {
      double t = 0.0;  // slices in order
      for (int s2 = 0; s2 < W; ++s2) t += part[s2 * A + lane];
      if (!ok) t = __builtin_nan("");
      if (slc == 0 && a.terminal_sum) a.terminal_sum[b * A + lane] = t;
      const float Tf = static_cast<float>(c[1]);
      const float F = static_cast<float>(c[4 + lane]) * math::exp_any(static_cast<float>(c[2] - c[4 + A + lane]) * Tf);
      pco[lane] = a.normalize ? F / static_cast<float>(t / static_cast<double>(P)) : 1.0f;
    }
    if (lane == 0) {
      // a failed exchange: NaN discount, so the targets are NaN (max(K - NaN, 0) alone would give 0)
      pco[A] = ok ? math::exp_any(static_cast<float>(-c[2]) * static_cast<float>(c[1])) : __builtin_nanf("");
      pco[A + 1] = static_cast<float>(c[0]);
      if (dyn && jj + 2 >= S) {  // the contract of iteration jj + 2 (slice 0 took it) and its coefficients
        const int64_t nb = ok ? get_sc1(reinterpret_cast<const int64_t*>(xs + W * A)) : a.B;
        bidx[(jj + 2) & 3] = nb;
        if (nb < a.B) coefs(nb, dco + ((jj + 2) & 1) * CS);
      }
    }
  };
  // step 2 (all waves, after a barrier that made pco visible): basket put of contract jj from the
  // terminal slots, column sums of the slice to the column buffer
  auto payoff = [&](int64_t jj) {
    float sc[A];
#pragma unroll
    for (int i = 0; i < A; ++i) sc[i] = pco[i];
    const float df = pco[A], Kf = pco[A + 1];
    const float wA = static_cast<float>(1.0 / A);
    v4f tv[A];
#pragma unroll
    for (int i = 0; i < A; ++i) tv[i] = term[i * kRThreads + tid];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float bs = 0.0f;
#pragma unroll
      for (int i = 0; i < A; ++i) bs = bs + tv[i][e] * sc[i];
      const float diff = Kf - bs * wA;
      part[g * N + 4 * q + e] = static_cast<double>(df * (diff > 0.0f ? diff : 0.0f));
    }
    lds_barrier();
    double* xc = xcol + (bof(jj) * W + slc) * static_cast<int64_t>(N);
    for (int n = tid; n < N; n += kRThreads) {
      double t = 0.0;
      for (int gg = 0; gg < G; ++gg) t += part[gg * N + n];
      xc[n] = t;
    }
  };

  const int64_t n_tab = dyn ? S : (a.B > grp ? (a.B - 1 - grp) / groups + 1 : 0);  // static iterations
  int64_t n_iter = 0;
  for (int64_t jj = 0;; ++jj) {
    const int64_t b = bof(jj);  // uniform (LDS ring, written before the last barrier)
    if (b >= a.B) break;
    n_iter = jj + 1;
    float* tab = table + ((jj / kRTable) & 1) * kRTable * CS;
    if (jj < n_tab && jj % kRTable == 0) {
      // wave 0 fills the coefficient table of the next 64 static contracts, one per lane
      const int64_t jl = jj + lane;
      if (wave == 0 && jl < n_tab) coefs(grp + jl * groups, tab + lane * CS);
      lds_barrier();
    }
    // 0. wave 0: contract jj - 1's scales (the other waves start simulating)
    if (jj > 0 && wave == 0) gather(jj - 1);
    const float* e = jj < n_tab ? tab + (jj % kRTable) * CS : dco + (jj & 1) * CS;
    float ca[A], x0[A], Lb[A][A];
#pragma unroll
    for (int i = 0; i < A; ++i) {
      ca[i] = e[i];
      x0[i] = e[A + i];
#pragma unroll
      for (int k = 0; k < A; ++k) Lb[i][k] = e[2 * A + i * A + k];
    }
    // 1. simulate: the lane's 4 paths of all A assets through the 16 rows
    const int64_t p0 = static_cast<int64_t>(slc) * kRChunk;
    const __amdgpu_buffer_rsrc_t crs = row_rsrc(a.paths + b * A * rows * a.pitch + p0);
    PathStream s(a.seed, static_cast<uint64_t>(ord0 + b), static_cast<uint64_t>(p0 / kBPaths + tid));
    float x[A][kBPaths];
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
      for (int j = 0; j < kBPaths; ++j) x[i][j] = x0[i];
    // a rolled row loop: unrolled, the compiler hoists all A x 16 row offsets into SGPRs and spills them
#pragma unroll 1
    for (int t = 0; t < kRowBlock; ++t) {
#pragma unroll
      for (int j = 0; j < kBPaths; j += 2) {
        float z0[A + 1], z1[A + 1];
#pragma unroll
        for (int k = 0; k < A; k += 2) s.template normal_pair<HW>(z0[k], z0[k + 1]);
#pragma unroll
        for (int k = 0; k < A; k += 2) s.template normal_pair<HW>(z1[k], z1[k + 1]);
#pragma unroll
        for (int i = 0; i < A; ++i) {
          f2 y = {ca[i], ca[i]};
#pragma unroll
          for (int k = 0; k <= i; ++k) y = __builtin_elementwise_fma(f2{Lb[i][k], Lb[i][k]}, f2{z0[k], z1[k]}, y);
          f2 ex;
          if constexpr (HW) ex = f2{__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)};
          else ex = f2{math::exp2_any(y.x), math::exp2_any(y.y)};
          const f2 xv = f2{x[i][j], x[i][j + 1]} * ex;
          x[i][j] = xv.x;
          x[i][j + 1] = xv.y;
        }
      }
      if (STORE_ALL || t == kRowBlock - 1) {
        // one descriptor per contract slice; the (asset, row) offset rides in the scalar offset
#pragma unroll
        for (int i = 0; i < A; ++i)
          __builtin_amdgcn_raw_buffer_store_b128(v4f{x[i][0], x[i][1], x[i][2], x[i][3]}, crs, lane_off,
                                                 static_cast<int>((i * rows + (STORE_ALL ? t : 0)) * pitch_b), 0);
      }
    }
    // this contract's slice sums: lane (f32 4-path partial -> f64), wave butterfly, waves in order
#pragma unroll
    for (int i = 0; i < A; ++i) {
      float p = 0.0f;
#pragma unroll
      for (int j = 0; j < kBPaths; ++j) p += x[i][j];
      const double w = bwave_sum(static_cast<double>(p));
      if (lane == 0) wsum[wave * A + i] = w;
    }
    lds_barrier();  // wsum of contract jj, scales of contract jj - 1
    // 2. contract jj - 1: payoffs and column sums (reads the terminal slots: own lane)
    if (jj > 0) payoff(jj - 1);
#pragma unroll
    for (int i = 0; i < A; ++i) term[i * kRThreads + tid] = v4f{x[i][0], x[i][1], x[i][2], x[i][3]};
    // 3. wave 0 publishes contract jj's slice sums: one drain, one arrival (the other waves go on)
    if (wave == 0) {
      if (lane < A) {
        double t = 0.0;
        for (int w2 = 0; w2 < kRWaves; ++w2) t += wsum[w2 * A + lane];
        put_sc1(xsum + (jj % kRSlots) * XS + slc * A + lane, t);
      }
      if (dyn && slc == 0 && lane == 0 && jj + 2 >= S)  // the group's contract of iteration jj + 2
        put_sc1(reinterpret_cast<int64_t*>(xsum + (jj % kRSlots) * XS + W * A), n_static + atomicAdd(queue, 1u));
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0 && !(ra.withhold && grp == 0 && slc == W - 1 && jj == 0))
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    lds_barrier();  // part / wsum are rewritten from here on
  }
  if (n_iter > 0) {  // the last contract
    if (wave == 0) gather(n_iter - 1);
    lds_barrier();
    payoff(n_iter - 1);
  }
  if (tid == 0) {
    // every workgroup made its last exchange before it arrives here: the last one resets the
    // group counters for the next launch
    __threadfence();
    uint32_t* done = reinterpret_cast<uint32_t*>(ra.sync);
    if (atomicAdd(done, 1u) == gridDim.x - 1) {
      for (int k = 0; k < groups; ++k) reinterpret_cast<uint32_t*>(ra.sync + 128 + 128 * static_cast<int64_t>(k))[0] = 0u;
      *queue = 0u;
      *launch_fail = 0u;
      *done = 0u;
    }
  }
}

// One workgroup per contract after basket_resident_kernel: the W slices' column sums added in
// slice order from 0.0, the M-mean and the FFT (fft_row) -> targets.
constexpr int kFThreads = 256;
__global__ __launch_bounds__(kFThreads) void basket_mean_fft_kernel(const double* __restrict__ xcol, int32_t W,
                                                                    int32_t N, int32_t M, float2* __restrict__ targets) {
  extern __shared__ double lds[];
  double* avg = lds;        // [N]
  double* cs = avg + N;     // [N]
  double* sn = cs + N;      // [N]
  double* xr = sn + N;      // [N]
  double* xi = xr + N;      // [N]
  const int64_t b = blockIdx.x;
  const double* xc = xcol + b * W * static_cast<int64_t>(N);
  for (int n = threadIdx.x; n < N; n += kFThreads) {
    math::twiddle(n, N, sn[n], cs[n]);
    double t = 0.0;
    for (int s2 = 0; s2 < W; ++s2) t += xc[static_cast<int64_t>(s2) * N + n];
    avg[n] = t / static_cast<double>(M);
  }
  __syncthreads();
  fft_row<float, kFThreads>(avg, cs, sn, N, xr, xi, targets + b * N);
}

size_t basket_lds_bytes(int A, int N) {
  const size_t part = static_cast<size_t>(N > 4 * kBThreads ? N : 4 * kBThreads);
  return (kMaxAssets * kMaxAssets + static_cast<size_t>(kBWaves) * A + A + part + 3 * static_cast<size_t>(N)) *
         sizeof(double);
}

size_t basket_cf_lds_bytes(int N) {
  const size_t part = static_cast<size_t>(N > 4 * kBThreads ? N : 4 * kBThreads);
  return (kMaxAssets + part + 3 * static_cast<size_t>(N)) * sizeof(double);
}

// Split (basket_kernel<1> then basket_cf_kernel) when the caller keeps the terminal sums: the CF
// re-read then streams at full read bandwidth instead of stalling each workgroup's store queue
// (as the single-asset paths_kernel + cf_kernel pair; kBasketSplit = false keeps the fused kernel)
constexpr bool kBasketSplit = true;

// ---- The host layer: one dispatch, one launch path, one mode rule and one argument screen for every kernel ----

// A run-time value as a compile-time constant: f is a generic callable and is handed a std::integral_constant.
// n_assets -> A in 1..8; any other count is "<entry>: n_assets must be in 1..8".
template <typename F>
auto with_assets(int n_assets, const char* entry, F&& f) -> decltype(f(std::integral_constant<int, 1>{})) {
  switch (n_assets) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: set_error("%s: n_assets must be in 1..8", entry); return SMC_ERR_INVALID_ARGUMENT;
  }
}

template <typename F>
auto with_flag(bool on, F&& f) -> decltype(f(std::true_type{})) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}

// (A, HW) of a call: f(A, HW), HW from math & SMC_MATH_HW
template <typename F>
auto with_variant(int n_assets, bool hw, const char* entry, F&& f) {
  return with_assets(n_assets, entry, [&](auto A) { return with_flag(hw, [&](auto HW) { return f(A, HW); }); });
}

template <typename F>
auto with_price_mode(int mode, F&& f) -> decltype(f(std::integral_constant<int, kBPriceRaw>{})) {
  return mode == kBPriceRaw   ? f(std::integral_constant<int, kBPriceRaw>{})
         : mode == kBPriceLds ? f(std::integral_constant<int, kBPriceLds>{})
                              : f(std::integral_constant<int, kBPriceReplay>{});
}

// One workgroup of kBThreads per contract with `lds` bytes of dynamic LDS (the limit raised where it is above 64 KiB).
template <typename K, typename... Args>
int32_t launch_per_contract(K kernel, const char* name, int64_t B, size_t lds, hipStream_t stream, Args... args) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: cannot raise the dynamic LDS limit", name);
    return SMC_ERR_HIP;
  }
  launch(kernel, dim3(static_cast<unsigned>(B)), dim3(kBThreads), static_cast<uint32_t>(lds), stream, args...);
  return check_launch(name);
}

template <int A, bool HW>
const void* basket_kernel_ptr() {
  return reinterpret_cast<const void*>(basket_kernel<A, HW, kBasketSplit ? 1 : 0>);
}

// Workgroups of the kernel launched for <A, HW, N> resident on the current device (occupancy x CUs).
template <int A, bool HW>
int64_t basket_slots_k(int N) {
  int dev = 0, cus = 0, per_cu = 0;
  const size_t lds = basket_lds_bytes(A, N);
  const void* kernel = basket_kernel_ptr<A, HW>();
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return (void)hipGetLastError(), -1;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess)
    return (void)hipGetLastError(), -1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBThreads, lds) != hipSuccess)
    return (void)hipGetLastError(), -1;
  return static_cast<int64_t>(per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
}

int64_t basket_slots(int n_assets, bool hw, int N) {
  if (n_assets < 1 || n_assets > kMaxAssets) return -1;
  return with_variant(n_assets, hw, "basket", [&](auto A, auto HW) { return basket_slots_k<A(), HW()>(N); });
}

template <int A, bool HW>
int32_t launch_basket_k(const BasketArgs& a, hipStream_t stream) {
  const size_t lds = basket_lds_bytes(A, a.N);
  if (!kBasketSplit || !a.terminal_sum)
    return launch_per_contract(basket_kernel<A, HW, 0>, "basket_kernel", a.B, lds, stream, a);
  if (int32_t st = launch_per_contract(basket_kernel<A, HW, 1>, "basket_kernel", a.B, lds, stream, a)) return st;
  return launch_per_contract(basket_cf_kernel<A>, "basket_cf_kernel", a.B, basket_cf_lds_bytes(a.N), stream, a);
}

int32_t launch_basket(int n_assets, bool hw, const BasketArgs& a, hipStream_t stream) {
  return with_variant(n_assets, hw, "basket", [&](auto A, auto HW) { return launch_basket_k<A(), HW()>(a, stream); });
}

// Workgroups per contract of basket_resident_kernel for this shape, or 0 when it does not take it
// (T = 16, N | 4096, 4 <= N <= 2048, P a multiple of 4096 and <= 32 x 4096, LDS within the CU's).
int basket_res_slices(int A, int T, int64_t N, int64_t M) {
  const int64_t P = N * M;
  if (T != kRowBlock || N < 4 || N > 2048 || N % 4 != 0 || kRChunk % N != 0 || P % kRChunk != 0) return 0;
  const int64_t W = P / kRChunk;
  if (W < 1 || W > kRMaxSlices || basket_resident_lds_bytes(A, static_cast<int>(N)) > 160 * 1024) return 0;
  return static_cast<int>(W);
}

// Contract sequences of the resident launch on the current device: floor(#CUs / W), -1 on failure.
int64_t basket_res_groups(int W) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return (void)hipGetLastError(), -1;
  return cus >= W ? cus / W : -1;
}

template <int A, bool HW>
int32_t launch_basket_resident_k(const BasketArgs& a, int W, int64_t groups, int64_t chunk, uint8_t* sync,
                                 hipStream_t stream) {
  const size_t lds = basket_resident_lds_bytes(A, a.N);
  auto kernel = a.store_all ? basket_resident_kernel<A, HW, true> : basket_resident_kernel<A, HW, false>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(lds)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SMC_ERR_HIP, "basket_resident_kernel: cannot raise the dynamic LDS limit");
  }
  const BasketSyncLayout l = basket_sync_layout(A, W, a.N, groups, chunk);
  const BasketResArgs ra{a, W, static_cast<int32_t>(groups), sync, l.xsum_off, l.xcol_off, exchange_spin_limit(),
                        exchange_fault().withhold};
  launch(kernel, dim3(static_cast<unsigned>(groups * W)), dim3(kRThreads), lds, stream, ra);
  if (int32_t st = check_launch("basket_resident_kernel")) return st;
  const size_t flds = 5 * static_cast<size_t>(a.N) * sizeof(double);
  if (flds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(basket_mean_fft_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(flds)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SMC_ERR_HIP, "basket_mean_fft_kernel: cannot raise the dynamic LDS limit");
  }
  launch(basket_mean_fft_kernel, dim3(static_cast<unsigned>(a.B)), dim3(kFThreads), flds, stream,
                     reinterpret_cast<const double*>(sync + l.xcol_off), W, a.N, a.M, a.targets);
  return check_launch("basket_mean_fft_kernel");
}

int32_t launch_basket_resident(int n_assets, bool hw, const BasketArgs& a, int W, int64_t groups, int64_t chunk,
                               uint8_t* sync, hipStream_t stream) {
  return with_variant(n_assets, hw, "basket", [&](auto A, auto HW) {
    return launch_basket_resident_k<A(), HW()>(a, W, groups, chunk, sync, stream);
  });
}

// What the five batched entry points share: the entry's name (for its messages) and the arguments all of them take.
struct BasketCall {
  const char* entry;
  const double* contracts;
  int64_t B;
  int32_t A, T;
  int64_t P;
  uint64_t seed;
  const int64_t* ordinal_dev;
  int64_t ordinal0;
  int32_t math, normalization;
};

int32_t fail_in(const char* entry, int32_t code, const char* what) {
  set_error("%s: %s", entry, what);
  return code;
}

// The shared checks, in the order every entry makes them; out_name names the entry's output block.
int32_t check_basket_call(const BasketCall& c, const char* out_name, const void* out) {
  if (!c.contracts) return fail_in(c.entry, SMC_ERR_INVALID_ARGUMENT, "contracts_dev is NULL");
  if (!out) {
    set_error("%s: %s is NULL", c.entry, out_name);
    return SMC_ERR_INVALID_ARGUMENT;
  }
  if (c.A < 1 || c.A > kMaxAssets) return fail_in(c.entry, SMC_ERR_INVALID_ARGUMENT, "n_assets must be in 1..8");
  if (c.math & ~(SMC_MATH_HW | SMC_PRICE_REPLAY))
    return fail_in(c.entry, SMC_ERR_INVALID_ARGUMENT, "bad math (0 or SMC_MATH_HW, optionally | SMC_PRICE_REPLAY)");
  if (c.normalization != SMC_NORM_RAW && c.normalization != SMC_NORM_NORMALIZE)
    return fail_in(c.entry, SMC_ERR_INVALID_ARGUMENT, "bad normalization");
  if (c.B < 0 || c.B > 0x7fffffffLL || c.T <= 0 || c.P <= 0)
    return fail_in(c.entry, SMC_ERR_INVALID_SHAPE, "need 0 <= n_contracts < 2^31, timesteps > 0, n_paths > 0");
  if (c.P >= (int64_t{1} << 40)) return fail_in(c.entry, SMC_ERR_INVALID_SHAPE, "n_paths too large (>= 2^40)");
  return SMC_OK;
}

int32_t check_basket_strides(const BasketCall& c, const double* weights, int64_t weights_stride, const double* corr,
                             int64_t corr_stride) {
  if (weights && weights_stride != 0 && weights_stride < c.A)
    return fail_in(c.entry, SMC_ERR_INVALID_ARGUMENT, "weights_stride must be 0 or >= n_assets");
  if (corr && corr_stride != 0 && corr_stride < c.A * (c.A - 1) / 2)
    return fail_in(c.entry, SMC_ERR_INVALID_ARGUMENT, "corr_stride must be 0 or >= n_assets (n_assets - 1) / 2");
  return SMC_OK;
}

BasketArgs basket_args(const BasketCall& c, double* terminal_sum) {
  BasketArgs a{};
  a.contracts = c.contracts;
  a.B = c.B;
  a.T = c.T;
  a.P = c.P;
  a.seed = c.seed;
  a.ordinal_dev = c.ordinal_dev;
  a.ordinal0 = c.ordinal0;
  a.normalize = c.normalization != SMC_NORM_RAW;
  a.terminal_sum = terminal_sum;
  return a;
}

BasketGeneralArgs basket_general_args(const BasketCall& c, const double* weights, int64_t weights_stride,
                                      const double* corr, int64_t corr_stride) {
  // A = 1 has no correlation entry: nothing to read, whatever the caller passed
  return BasketGeneralArgs{weights, weights_stride, c.A > 1 ? corr : nullptr, corr_stride};
}

// The screen of every plan below (host only, no HIP call): a shape and flags the batched kernels take.
bool basket_plan_ok(int A, int64_t P, int32_t math, int32_t normalization) {
  if (A < 1 || A > kMaxAssets || P <= 0 || P >= (int64_t{1} << 40)) return false;
  if (math & ~(SMC_MATH_HW | SMC_PRICE_REPLAY)) return false;
  return normalization == SMC_NORM_RAW || normalization == SMC_NORM_NORMALIZE;
}

// A kernel under the raw / lds / replay rule: its name, the scratch bytes at the head of its dynamic LDS and what
// its smc_*_kernel entry reports per mode (BasketPriceMode's order).
struct ParkKernel {
  const char* name;
  size_t scratch;
  const char* mode_name[3];
};
constexpr ParkKernel kParkPrice{"basket_price_kernel", kBPriceScratch,
                                {"basket_price_kernel(raw)", "basket_price_kernel(lds)", "basket_price_kernel(replay)"}};
constexpr ParkKernel kParkGeneral{
    "basket_general_kernel", kBGeneralScratch,
    {"basket_general_kernel(raw)", "basket_general_kernel(lds)", "basket_general_kernel(replay)"}};
constexpr ParkKernel kParkGreeks{
    "basket_greeks_kernel", kBGreekScratch,
    {"basket_greeks_kernel(raw)", "basket_greeks_kernel(lds)", "basket_greeks_kernel(replay)"}};
constexpr ParkKernel kParkGreeksGeneral{
    "basket_greeks_general_kernel", kBGGScratch,
    {"basket_greeks_general_kernel(raw)", "basket_greeks_general_kernel(lds)", "basket_greeks_general_kernel(replay)"}};

// A ParkKernel's mode and dynamic LDS for a shape (host only, no HIP call); -1: not a call it takes.
// math: 0 or SMC_MATH_HW, optionally | SMC_PRICE_REPLAY.  NORMALIZE parks the terminal values in LDS while the
// scratch and [A][P rounded up to 4] floats fit kBPriceParkBytes, and replays the streams beyond.
int basket_park_mode(const ParkKernel& k, int A, int64_t P, int32_t math, int32_t normalization, size_t* lds) {
  if (!basket_plan_ok(A, P, math, normalization)) return -1;
  *lds = k.scratch;
  if (normalization == SMC_NORM_RAW) return kBPriceRaw;
  if (math & SMC_PRICE_REPLAY) return kBPriceReplay;
  const size_t park = k.scratch + static_cast<size_t>(A) * ((static_cast<size_t>(P) + 3) & ~size_t{3}) * sizeof(float);
  if (park > kBPriceParkBytes) return kBPriceReplay;
  *lds = park;
  return kBPriceLds;
}

const char* park_kernel_name(const ParkKernel& k, int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                             int32_t normalization) {
  size_t lds = 0;
  if (timesteps <= 0) return "unsupported";
  const int mode = basket_park_mode(k, n_assets, n_paths, math, normalization, &lds);
  return mode < 0 ? "unsupported" : k.mode_name[mode];
}

// The launch of a checked call of a ParkKernel: pick(A, HW, MODE) names the kernel's instance, args follow `a`.
template <typename Pick, typename... Args>
int32_t launch_parked(const BasketCall& c, const ParkKernel& k, hipStream_t stream, Pick pick, Args... args) {
  size_t lds = 0;
  const int mode = basket_park_mode(k, c.A, c.P, c.math, c.normalization, &lds);
  return with_variant(c.A, c.math & SMC_MATH_HW, c.entry, [&](auto A, auto HW) {
    return with_price_mode(mode, [&](auto MODE) {
      return launch_per_contract(pick(A, HW, MODE), k.name, c.B, lds, stream, args...);
    });
  });
}

// basket_path_kernel's plan for a shape (host only, no HIP call): 0 one RAW simulation per column group, 1 the
// NORMALIZE replay, -1 not a call it takes, -2 more scales (A T) than LDS holds beside one date of accumulators.
// *dates is the number of whole time rows per sweep (NORMALIZE), *lds the dynamic LDS.
int basket_path_plan(int A, int32_t T, int64_t P, int32_t math, int32_t normalization, size_t* lds, int* dates) {
  if (T <= 0 || !basket_plan_ok(A, P, math, normalization)) return -1;
  *dates = 0;
  *lds = kBPathScratch + static_cast<size_t>(A) * kBPathAccRow;
  if (normalization == SMC_NORM_RAW) return 0;
  const size_t head = kBPathScratch + ((static_cast<size_t>(A) * static_cast<size_t>(T) * sizeof(float) + 7) & ~size_t{7});
  if (head + static_cast<size_t>(A) * kBPathAccRow > kBPathLdsBytes) return -2;
  const size_t fit = (kBPathLdsBytes - head) / kBPathAccRow / static_cast<size_t>(A);  // >= 1
  *dates = static_cast<int>(static_cast<size_t>(T) < fit ? static_cast<size_t>(T) : fit);
  *lds = head + static_cast<size_t>(*dates) * A * kBPathAccRow;
  return 1;
}

// basket_path_greeks_kernel's plan for a shape (host only, no HIP call): 0 the RAW passes, 1 the NORMALIZE replay,
// -1 not a call it takes, -2 row tables (3 A + 1 f32 per date) that leave no room for one date of accumulators (2 A
// rows), in either normalisation.  *dates is the number of whole time rows per sweep (NORMALIZE), *lds the dynamic LDS.
int basket_path_greeks_plan(int A, int32_t T, int64_t P, int32_t math, int32_t normalization, size_t* lds, int* dates) {
  if (T <= 0 || !basket_plan_ok(A, P, math, normalization)) return -1;
  *dates = 0;
  const size_t date = 2 * static_cast<size_t>(A) * kBPathAccRow;
  const size_t tables = static_cast<size_t>(3 * A + 1) * static_cast<size_t>(T) * sizeof(float);
  if (tables > kBPathLdsBytes) return -2;
  const size_t head = kBPGScratch + ((tables + 7) & ~size_t{7});
  *lds = head;
  if (head + date > kBPathLdsBytes) return -2;
  if (normalization == SMC_NORM_RAW) return 0;
  const size_t fit = (kBPathLdsBytes - head) / date;  // >= 1
  *dates = static_cast<int>(static_cast<size_t>(T) < fit ? static_cast<size_t>(T) : fit);
  *lds = head + static_cast<size_t>(*dates) * date;
  return 1;
}

}  // namespace
}  // namespace smc

using namespace smc;

extern "C" {
#pragma GCC visibility push(default)
int32_t smc_basket_train_targets(const double* contracts_dev, int64_t n_contracts, int32_t n_assets,
                                 int32_t timesteps, int32_t network_size, int32_t batches_per_mc_run,
                                 uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                                 int32_t normalization, int32_t store_mode, void* paths_dev, int64_t path_pitch,
                                 int64_t chunk_contracts, double* terminal_sum_dev, void* targets_dev,
                                 void* sync_dev, int64_t sync_bytes, void* stream) {
  const int64_t N = network_size, M = batches_per_mc_run, P = N * M;
  if (!contracts_dev || !paths_dev || !targets_dev)
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_basket_train_targets: NULL buffer");
  if (n_assets < 1 || n_assets > kMaxAssets)
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_basket_train_targets: n_assets must be in 1..8");
  if (n_contracts < 0 || n_contracts > 0x7fffffffLL || timesteps <= 0 || N <= 0 || M <= 0)
    return fail(SMC_ERR_INVALID_SHAPE, "smc_basket_train_targets: need 0 <= B < 2^31, T > 0, N > 0, M > 0");
  if (N % 4 != 0 || N > 4096 || P % kBChunk != 0 || P >= (int64_t{1} << 29))
    return fail(SMC_ERR_INVALID_SHAPE,
                "smc_basket_train_targets: need N % 4 == 0, N <= 4096, N*M a multiple of 2048 and < 2^29");
  if (math != 0 && math != SMC_MATH_HW) return fail(SMC_ERR_INVALID_ARGUMENT, "smc_basket_train_targets: bad math");
  if (store_mode != SMC_STORE_ALL && store_mode != SMC_STORE_TERMINAL)
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_basket_train_targets: bad store_mode");
  if (path_pitch != 0 && (path_pitch < P || path_pitch % 4 != 0))
    return fail(SMC_ERR_INVALID_SHAPE, "smc_basket_train_targets: path_pitch must be 0 or a multiple of 4 >= P");
  if (chunk_contracts <= 0) return fail(SMC_ERR_INVALID_ARGUMENT, "smc_basket_train_targets: chunk_contracts <= 0");
  if (basket_lds_bytes(n_assets, static_cast<int>(N)) > 160 * 1024)
    return fail(SMC_ERR_INVALID_SHAPE, "smc_basket_train_targets: network_size exceeds the LDS budget");
  const int64_t width = 3 * n_assets + 4;
  // resident kernel where the shape allows and the caller passed a sync area of the right size
  const int64_t rows_all = store_mode == SMC_STORE_ALL ? timesteps : 1;
  const int64_t block_bytes = n_assets * rows_all * (path_pitch ? path_pitch : P) * 4;
  const int W = sync_dev && block_bytes < (int64_t{1} << 31) ? basket_res_slices(n_assets, timesteps, N, M) : 0;
  int64_t groups = 0;
  if (W > 0) {
    groups = basket_res_groups(W);
    if (groups <= 0) return fail(SMC_ERR_HIP, "smc_basket_train_targets: device query failed");
    // a CU-masked stream (the data-parallel step keeps its collective and network kernels on CUs of their own):
    // only as many groups as the stream's CUs hold, so every workgroup of a group is resident at once
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return (void)hipGetLastError(), fail(SMC_ERR_HIP, "smc_basket_train_targets: device query failed");
    const int64_t on_stream = stream_cus(as_stream(stream), cus) / W;
    if (on_stream <= 0) return fail(SMC_ERR_INVALID_SHAPE, "smc_basket_train_targets: fewer CUs on the stream than slices");
    if (on_stream < groups) groups = on_stream;
    if (sync_bytes < basket_sync_layout(n_assets, W, static_cast<int>(N), groups, chunk_contracts).bytes)
      return fail(SMC_ERR_INVALID_ARGUMENT, "smc_basket_train_targets: sync_bytes < smc_basket_sync_bytes(...)");
  }
  for (int64_t off = 0; off < n_contracts; off += chunk_contracts) {
    const int64_t nb = n_contracts - off < chunk_contracts ? n_contracts - off : chunk_contracts;
    BasketArgs a{contracts_dev + off * width, nb, timesteps, P, network_size, batches_per_mc_run, mc_seed,
                 ordinal_dev, ordinal0 + off, normalization != SMC_NORM_RAW, store_mode == SMC_STORE_ALL,
                 static_cast<float*>(paths_dev), path_pitch ? path_pitch : P,
                 terminal_sum_dev ? terminal_sum_dev + off * n_assets : nullptr,
                 static_cast<float2*>(targets_dev) + off * N};
    uint8_t* sync = static_cast<uint8_t*>(sync_dev);
    const bool hw = math == SMC_MATH_HW;
    const int32_t st =
        W > 0 ? launch_basket_resident(n_assets, hw, a, W, groups, chunk_contracts, sync, as_stream(stream))
              : launch_basket(n_assets, hw, a, as_stream(stream));
    if (st) return st;
  }
  return SMC_OK;
}

int64_t smc_basket_sync_bytes(int32_t n_assets, int32_t timesteps, int32_t network_size, int32_t batches_per_mc_run,
                              int64_t chunk_contracts) {
  if (n_assets < 1 || n_assets > kMaxAssets || network_size <= 0 || batches_per_mc_run <= 0 || chunk_contracts <= 0)
    return -1;
  const int W = basket_res_slices(n_assets, timesteps, network_size, batches_per_mc_run);
  if (W == 0) return 0;
  const int64_t groups = basket_res_groups(W);
  if (groups <= 0) return -1;
  return basket_sync_layout(n_assets, W, network_size, groups, chunk_contracts).bytes;
}

const char* smc_basket_train_targets_kernel(int32_t n_assets, int32_t timesteps, int32_t network_size,
                                            int32_t batches_per_mc_run, int32_t with_sync, int32_t keep_sums) {
  if (with_sync && n_assets >= 1 && n_assets <= kMaxAssets && network_size > 0 && batches_per_mc_run > 0 &&
      basket_res_slices(n_assets, timesteps, network_size, batches_per_mc_run) > 0)
    return "basket_resident_kernel";
  return keep_sums && kBasketSplit ? "basket_kernel+basket_cf_kernel" : "basket_kernel";
}

int64_t smc_basket_resident_slots(int32_t n_assets, int32_t network_size, int32_t math) {
  if (n_assets < 1 || n_assets > kMaxAssets || network_size <= 0 || network_size > 4096) return -1;
  return basket_slots(n_assets, math == SMC_MATH_HW, network_size);
}

int32_t smc_basket_price(const double* contracts_dev, int64_t n_contracts, int32_t n_assets, int32_t timesteps,
                         int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                         int32_t normalization, double* prices_dev, double* terminal_sum_dev, void* stream) {
  const BasketCall c{"smc_basket_price", contracts_dev, n_contracts, n_assets, timesteps, n_paths,
                     mc_seed, ordinal_dev, ordinal0, math, normalization};
  if (int32_t st = check_basket_call(c, "prices_dev", prices_dev)) return st;
  if (n_contracts == 0) return SMC_OK;
  const auto pick = [](auto A, auto HW, auto MODE) { return basket_price_kernel<A(), HW(), MODE()>; };
  return launch_parked(c, kParkPrice, as_stream(stream), pick, basket_args(c, terminal_sum_dev), prices_dev);
}

const char* smc_basket_price_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                    int32_t normalization) {
  return park_kernel_name(kParkPrice, n_assets, timesteps, n_paths, math, normalization);
}

int32_t smc_basket_price_general(const double* contracts_dev, const double* weights_dev, int64_t weights_stride,
                                 const double* corr_dev, int64_t corr_stride, int64_t n_contracts, int32_t n_assets,
                                 int32_t timesteps, int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                                 int64_t ordinal0, int32_t math, int32_t normalization, double* prices_dev,
                                 double* terminal_sum_dev, void* stream) {
  const BasketCall c{"smc_basket_price_general", contracts_dev, n_contracts, n_assets, timesteps, n_paths,
                     mc_seed, ordinal_dev, ordinal0, math, normalization};
  if (int32_t st = check_basket_call(c, "prices_dev", prices_dev)) return st;
  if (int32_t st = check_basket_strides(c, weights_dev, weights_stride, corr_dev, corr_stride)) return st;
  if (n_contracts == 0) return SMC_OK;
  const auto pick = [](auto A, auto HW, auto MODE) { return basket_general_kernel<A(), HW(), MODE()>; };
  return launch_parked(c, kParkGeneral, as_stream(stream), pick, basket_args(c, terminal_sum_dev),
                       basket_general_args(c, weights_dev, weights_stride, corr_dev, corr_stride), prices_dev);
}

const char* smc_basket_price_general_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                            int32_t normalization) {
  return park_kernel_name(kParkGeneral, n_assets, timesteps, n_paths, math, normalization);
}

int32_t smc_basket_greeks(const double* contracts_dev, int64_t n_contracts, int32_t n_assets, int32_t timesteps,
                          int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                          int32_t normalization, double* greeks_dev, double* sums_dev, void* stream) {
  const BasketCall c{"smc_basket_greeks", contracts_dev, n_contracts, n_assets, timesteps, n_paths,
                     mc_seed, ordinal_dev, ordinal0, math, normalization};
  if (int32_t st = check_basket_call(c, "greeks_dev", greeks_dev)) return st;
  if (n_contracts == 0) return SMC_OK;
  const auto pick = [](auto A, auto HW, auto MODE) { return basket_greeks_kernel<A(), HW(), MODE()>; };
  return launch_parked(c, kParkGreeks, as_stream(stream), pick, basket_args(c, nullptr), greeks_dev, sums_dev);
}

const char* smc_basket_greeks_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                     int32_t normalization) {
  return park_kernel_name(kParkGreeks, n_assets, timesteps, n_paths, math, normalization);
}

int32_t smc_basket_greeks_cols(int32_t n_assets) {
  return n_assets < 1 || n_assets > kMaxAssets ? -1 : 8 * n_assets + 16;
}

int32_t smc_basket_greeks_general(const double* contracts_dev, const double* weights_dev, int64_t weights_stride,
                                  const double* corr_dev, int64_t corr_stride, int64_t n_contracts, int32_t n_assets,
                                  int32_t timesteps, int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                                  int64_t ordinal0, int32_t math, int32_t normalization, double* greeks_dev,
                                  double* sums_dev, void* stream) {
  const BasketCall c{"smc_basket_greeks_general", contracts_dev, n_contracts, n_assets, timesteps, n_paths,
                     mc_seed, ordinal_dev, ordinal0, math, normalization};
  if (int32_t st = check_basket_call(c, "greeks_dev", greeks_dev)) return st;
  if (int32_t st = check_basket_strides(c, weights_dev, weights_stride, corr_dev, corr_stride)) return st;
  if (n_contracts == 0) return SMC_OK;
  const auto pick = [](auto A, auto HW, auto MODE) { return basket_greeks_general_kernel<A(), HW(), MODE()>; };
  return launch_parked(c, kParkGreeksGeneral, as_stream(stream), pick, basket_args(c, nullptr),
                       basket_general_args(c, weights_dev, weights_stride, corr_dev, corr_stride), greeks_dev, sums_dev);
}

const char* smc_basket_greeks_general_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                             int32_t normalization) {
  return park_kernel_name(kParkGreeksGeneral, n_assets, timesteps, n_paths, math, normalization);
}

int32_t smc_basket_greeks_general_cols(int32_t n_assets) {
  return n_assets < 1 || n_assets > kMaxAssets ? -1 : 2 * n_assets * n_assets + 6 * n_assets + 12;
}

int32_t smc_basket_price_paths(const double* contracts_dev, const double* weights_dev, int64_t weights_stride,
                               const double* corr_dev, int64_t corr_stride, const double* barriers_dev,
                               int64_t n_contracts, int32_t n_assets, int32_t timesteps, int64_t n_paths,
                               uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                               int32_t normalization, double* prices_dev, double* terminal_sum_dev, void* stream) {
  const BasketCall c{"smc_basket_price_paths", contracts_dev, n_contracts, n_assets, timesteps, n_paths,
                     mc_seed, ordinal_dev, ordinal0, math, normalization};
  if (int32_t st = check_basket_call(c, "prices_dev", prices_dev)) return st;
  if (int32_t st = check_basket_strides(c, weights_dev, weights_stride, corr_dev, corr_stride)) return st;
  size_t lds = 0;
  int dates = 0;
  if (basket_path_plan(n_assets, timesteps, n_paths, math, normalization, &lds, &dates) < 0)
    return fail(SMC_ERR_INVALID_SHAPE,
                "smc_basket_price_paths: n_assets * timesteps scales do not fit the LDS table (SMC_NORM_NORMALIZE)");
  if (n_contracts == 0) return SMC_OK;
  const BasketArgs a = basket_args(c, terminal_sum_dev);
  const BasketGeneralArgs g = basket_general_args(c, weights_dev, weights_stride, corr_dev, corr_stride);
  const auto pick = [](auto A, auto HW, auto NORM) { return basket_path_kernel<A(), HW(), NORM()>; };
  return with_variant(n_assets, math & SMC_MATH_HW, c.entry, [&](auto A, auto HW) {
    return with_flag(a.normalize, [&](auto NORM) {
      return launch_per_contract(pick(A, HW, NORM), "basket_path_kernel", c.B, lds, as_stream(stream), a, g,
                                 barriers_dev, prices_dev, dates);
    });
  });
}

const char* smc_basket_price_paths_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                          int32_t normalization) {
  size_t lds = 0;
  int dates = 0;
  switch (basket_path_plan(n_assets, timesteps, n_paths, math, normalization, &lds, &dates)) {
    case 0: return "basket_path_kernel(raw)";
    case 1: return "basket_path_kernel(replay)";
    default: return "unsupported";
  }
}

int32_t smc_basket_greeks_paths(const double* contracts_dev, const double* weights_dev, int64_t weights_stride,
                                const double* corr_dev, int64_t corr_stride, int64_t n_contracts, int32_t n_assets,
                                int32_t timesteps, int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                                int64_t ordinal0, int32_t math, int32_t normalization, double* greeks_dev,
                                void* stream) {
  const BasketCall c{"smc_basket_greeks_paths", contracts_dev, n_contracts, n_assets, timesteps, n_paths,
                     mc_seed, ordinal_dev, ordinal0, math, normalization};
  if (int32_t st = check_basket_call(c, "greeks_dev", greeks_dev)) return st;
  if (int32_t st = check_basket_strides(c, weights_dev, weights_stride, corr_dev, corr_stride)) return st;
  size_t lds = 0;
  int dates = 0;
  if (basket_path_greeks_plan(n_assets, timesteps, n_paths, math, normalization, &lds, &dates) < 0)
    return fail(SMC_ERR_INVALID_SHAPE,
                "smc_basket_greeks_paths: the row tables of n_assets * timesteps leave no room for one date of "
                "accumulators in LDS");
  if (n_contracts == 0) return SMC_OK;
  const BasketArgs a = basket_args(c, nullptr);
  const BasketGeneralArgs g = basket_general_args(c, weights_dev, weights_stride, corr_dev, corr_stride);
  const auto pick = [](auto A, auto HW, auto NORM) { return basket_path_greeks_kernel<A(), HW(), NORM()>; };
  return with_variant(n_assets, math & SMC_MATH_HW, c.entry, [&](auto A, auto HW) {
    return with_flag(a.normalize, [&](auto NORM) {
      return launch_per_contract(pick(A, HW, NORM), "basket_path_greeks_kernel", c.B, lds, as_stream(stream), a, g,
                                 greeks_dev, dates);
    });
  });
}

const char* smc_basket_greeks_paths_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                           int32_t normalization) {
  size_t lds = 0;
  int dates = 0;
  switch (basket_path_greeks_plan(n_assets, timesteps, n_paths, math, normalization, &lds, &dates)) {
    case 0: return "basket_path_greeks_kernel(raw)";
    case 1: return "basket_path_greeks_kernel(replay)";
    default: return "unsupported";
  }
}

int32_t smc_basket_greeks_paths_cols(int32_t n_assets) {
  return n_assets < 1 || n_assets > kMaxAssets ? -1 : 16 * n_assets + 24;
}

#pragma GCC visibility pop
}  // extern "C"

