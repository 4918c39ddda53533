// smc_test_math_eval (spectralmc_hip_testing.h): the device math functions of smc_math.h and the Box-Muller
// arithmetic of smc_rng.h evaluated elementwise at caller-chosen inputs, so tests can sweep their whole input
// domains (tests/test_gpu_math.py).  The kernel calls the functions the engines call; nothing is restated here.
#include "../../include/spectralmc_hip_testing.h"
#include "smc_internal.h"
#include "smc_math.h"
#include "smc_rng.h"

namespace smc {
namespace {

constexpr int kEvalThreads = 256;
constexpr int64_t kEvalMaxBlocks = 2048;  // grid-stride beyond: the f64 functions load 51 KB of tables per block

template <int FN>
constexpr bool kUsesF64Tables = FN == SMC_TEST_MATH_M2LOG_U32 || FN == SMC_TEST_MATH_SINCOS_U32 ||
                                FN == SMC_TEST_MATH_EXP2S || FN == SMC_TEST_MATH_MUL_EXP2S ||
                                FN == SMC_TEST_MATH_NORMAL_F64;

// Element i of function FN (layouts: spectralmc_hip_testing.h); i < n is the caller's check.
template <int FN>
__device__ __forceinline__ void eval_one(const void* in, void* out, int64_t i) {
  const float* fi = static_cast<const float*>(in);
  const uint32_t* ui = static_cast<const uint32_t*>(in);
  const double* di = static_cast<const double*>(in);
  const int64_t* li = static_cast<const int64_t*>(in);
  float* fo = static_cast<float*>(out);
  double* dout = static_cast<double*>(out);
  if constexpr (FN == SMC_TEST_MATH_LOG_POS) {
    fo[i] = math::log_pos(fi[i]);
  } else if constexpr (FN == SMC_TEST_MATH_SINCOS_U24) {
    float s, c;
    math::sincos2pi_u24(ui[i], s, c);
    fo[2 * i] = s;
    fo[2 * i + 1] = c;
  } else if constexpr (FN == SMC_TEST_MATH_EXP2_ANY) {
    fo[i] = math::exp2_any(fi[i]);
  } else if constexpr (FN == SMC_TEST_MATH_EXP_ANY) {
    fo[i] = math::exp_any(fi[i]);
  } else if constexpr (FN == SMC_TEST_MATH_NORMAL_F32 || FN == SMC_TEST_MATH_NORMAL_F32_HW) {
    constexpr bool HW = FN == SMC_TEST_MATH_NORMAL_F32_HW;
    const float zs = static_cast<float>(PathStream::kNormalScale<HW>);  // as normals_kernel
    float z0, z1;
    PathStream::box_muller<HW>(ui[2 * i], ui[2 * i + 1], z0, z1);
    fo[2 * i] = zs * z0;
    fo[2 * i + 1] = zs * z1;
  } else if constexpr (FN == SMC_TEST_MATH_HW_INCREMENT) {
    float y0, y1;
    PathStream::hw_log_pair(ui[2 + 2 * i], ui[2 + 2 * i + 1], fi[0], fi[1], y0, y1);
    fo[2 * i] = y0;
    fo[2 * i + 1] = y1;
  } else if constexpr (FN == SMC_TEST_MATH_HW_EXP2) {
    fo[i] = __builtin_amdgcn_exp2f(fi[i]);
  } else if constexpr (FN == SMC_TEST_MATH_HW_LOG) {
    fo[i] = math::hw_log(fi[i]);
  } else if constexpr (FN == SMC_TEST_MATH_M2LOG_U32) {
    dout[i] = math::m2log_u32(ui[i]);
  } else if constexpr (FN == SMC_TEST_MATH_SQRT_RADIUS) {
    dout[i] = math::sqrt_radius(di[i]);
  } else if constexpr (FN == SMC_TEST_MATH_SINCOS_U32) {
    double s, c;
    math::sincos2pi_u32(ui[i], s, c);
    dout[2 * i] = s;
    dout[2 * i + 1] = c;
  } else if constexpr (FN == SMC_TEST_MATH_EXP2S) {
    dout[i] = math::exp2s_f64(di[i]);
  } else if constexpr (FN == SMC_TEST_MATH_MUL_EXP2S) {
    dout[i] = math::mul_exp2s_f64(di[2 * i], di[2 * i + 1]);
  } else if constexpr (FN == SMC_TEST_MATH_NORMAL_F64) {
    double z0, z1;
    PathStream::box_muller(ui[2 * i], ui[2 * i + 1], z0, z1);
    dout[2 * i] = z0;
    dout[2 * i + 1] = z1;
  } else {
    static_assert(FN == SMC_TEST_MATH_TWIDDLE, "unknown function id");
    double s, c;
    math::twiddle(li[2 * i], li[2 * i + 1], s, c);
    dout[2 * i] = s;
    dout[2 * i + 1] = c;
  }
}

template <int FN>
__global__ __launch_bounds__(kEvalThreads) void math_eval_kernel(const void* __restrict__ in, int64_t n,
                                                                 void* __restrict__ out) {
  if constexpr (kUsesF64Tables<FN>) math::f64_tables_load();  // before any thread leaves
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    eval_one<FN>(in, out, i);
}

template <int FN>
void launch_eval(const void* in, int64_t n, void* out, hipStream_t stream) {
  int64_t blocks = (n + kEvalThreads - 1) / kEvalThreads;
  if (blocks > kEvalMaxBlocks) blocks = kEvalMaxBlocks;
  launch_aux((math_eval_kernel<FN>), dim3(static_cast<unsigned>(blocks)), dim3(kEvalThreads), 0, stream, in, n, out);
}

}  // namespace
}  // namespace smc

extern "C" {
#pragma GCC visibility push(default)

int32_t smc_test_math_eval(int32_t fn, const void* in_dev, int64_t n, void* out_dev, void* stream) {
  using namespace smc;
  if (!test_hooks_enabled())
    return fail(SMC_ERR_INVALID_ARGUMENT, "smc_test_math_eval: test hooks disabled (SMC_ENABLE_TEST_HOOKS=1)");
  if (!in_dev || !out_dev) return fail(SMC_ERR_INVALID_ARGUMENT, "smc_test_math_eval: NULL pointer");
  if (n < 0) return fail(SMC_ERR_INVALID_SHAPE, "smc_test_math_eval: n < 0");
  if (fn < 0 || fn >= SMC_TEST_MATH_COUNT) return fail(SMC_ERR_INVALID_ARGUMENT, "smc_test_math_eval: bad function id");
  if (n == 0) return SMC_OK;
  const hipStream_t s = as_stream(stream);
  switch (fn) {
#define SMC_EVAL_CASE(id) \
  case id:                \
    launch_eval<id>(in_dev, n, out_dev, s); \
    break;
    SMC_EVAL_CASE(SMC_TEST_MATH_LOG_POS)
    SMC_EVAL_CASE(SMC_TEST_MATH_SINCOS_U24)
    SMC_EVAL_CASE(SMC_TEST_MATH_EXP2_ANY)
    SMC_EVAL_CASE(SMC_TEST_MATH_EXP_ANY)
    SMC_EVAL_CASE(SMC_TEST_MATH_NORMAL_F32)
    SMC_EVAL_CASE(SMC_TEST_MATH_NORMAL_F32_HW)
    SMC_EVAL_CASE(SMC_TEST_MATH_HW_INCREMENT)
    SMC_EVAL_CASE(SMC_TEST_MATH_HW_EXP2)
    SMC_EVAL_CASE(SMC_TEST_MATH_HW_LOG)
    SMC_EVAL_CASE(SMC_TEST_MATH_M2LOG_U32)
    SMC_EVAL_CASE(SMC_TEST_MATH_SQRT_RADIUS)
    SMC_EVAL_CASE(SMC_TEST_MATH_SINCOS_U32)
    SMC_EVAL_CASE(SMC_TEST_MATH_EXP2S)
    SMC_EVAL_CASE(SMC_TEST_MATH_MUL_EXP2S)
    SMC_EVAL_CASE(SMC_TEST_MATH_NORMAL_F64)
    SMC_EVAL_CASE(SMC_TEST_MATH_TWIDDLE)
#undef SMC_EVAL_CASE
  }
  return check_launch("math_eval_kernel");
}

#pragma GCC visibility pop
}  // extern "C"
