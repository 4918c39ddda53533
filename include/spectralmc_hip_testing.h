/*
 * spectralmc_hip_testing.h — test-only entry points of libspectralmc_hip.so (not part of the product
 * ABI in spectralmc_hip.h; no reference seam).
 *
 * They are inert unless the process environment holds SMC_ENABLE_TEST_HOOKS=1 when the first of them is
 * called (tests/conftest.py sets it); otherwise they change nothing and return SMC_ERR_INVALID_ARGUMENT.
 */
#ifndef SPECTRALMC_HIP_TESTING_H
#define SPECTRALMC_HIP_TESTING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Exchange fault injection (tests/test_gpu_engine.py, tests/test_gpu_basket.py): for the exchanging
 * launches enqueued after this call, withhold = 1 makes slice W-1 of group 0 skip its first arrival (its
 * partners time out), and spin_limit (> 0) replaces the ~1 s poll budget.  (0, 0) restores normal
 * operation. */
int32_t smc_test_exchange_fault(int32_t withhold, uint32_t spin_limit);

/* Elementwise evaluation of one device math function (tests/test_gpu_math.py): out[i] = fn(in[i]) for i < n,
 * one 256-thread grid-stride kernel on `stream` that calls the function the engines call (csrc/smc_math.h,
 * csrc/smc_rng.h).  fn fixes the element types; pairs are interleaved (element i at [2 i], [2 i + 1]).
 *
 *   id                in (per element)           out (per element)   device function
 *   LOG_POS           f32 u (positive normal)    f32                 math::log_pos
 *   SINCOS_U24        u32 j < 2^24               f32 x 2 (sin, cos)  math::sincos2pi_u24
 *   EXP2_ANY          f32                        f32                 math::exp2_any
 *   EXP_ANY           f32                        f32                 math::exp_any
 *   NORMAL_F32        u32 x 2 (a, b)             f32 x 2 (z0, z1)    PathStream::box_muller<false> (normal_pair<false>)
 *   NORMAL_F32_HW     u32 x 2 (a, b)             f32 x 2 (z0, z1)    PathStream::box_muller<true> times kNormalScale<true>,
 *                                                                    as normals_kernel stores it
 *   HW_INCREMENT      u32 x 2 (a, b)             f32 x 2 (ylo, yhi)  PathStream::hw_log_pair: ca + (cb r) (cos, sin); the
 *                     after two f32 (cb, ca) at the head of `in`     coefficients are in[0], in[1], the pairs start at in[2]
 *   HW_EXP2           f32                        f32                 __builtin_amdgcn_exp2f (v_exp_f32)
 *   HW_LOG            f32                        f32                 math::hw_log (v_log_f32 times ln 2)
 *   M2LOG_U32         u32                        f64                 math::m2log_u32
 *   SQRT_RADIUS       f64 in [2.3e-10, 46.1]     f64                 math::sqrt_radius
 *   SINCOS_U32        u32                        f64 x 2 (sin, cos)  math::sincos2pi_u32
 *   EXP2S             f64 ys                     f64                 math::exp2s_f64
 *   MUL_EXP2S         f64 x 2 (x, ys)            f64                 math::mul_exp2s_f64
 *   NORMAL_F64        u32 x 2 (a, b)             f64 x 2 (z0, z1)    PathStream::box_muller (normal_pair, f64)
 *   TWIDDLE           i64 x 2 (j, N), N > 0      f64 x 2 (sin, cos)  math::twiddle
 *
 * n = 0 is a no-op.  SMC_ERR_INVALID_ARGUMENT: hooks disabled, NULL pointer, unknown id; SMC_ERR_INVALID_SHAPE: n < 0. */
enum {
  SMC_TEST_MATH_LOG_POS = 0,
  SMC_TEST_MATH_SINCOS_U24 = 1,
  SMC_TEST_MATH_EXP2_ANY = 2,
  SMC_TEST_MATH_EXP_ANY = 3,
  SMC_TEST_MATH_NORMAL_F32 = 4,
  SMC_TEST_MATH_NORMAL_F32_HW = 5,
  SMC_TEST_MATH_HW_INCREMENT = 6,
  SMC_TEST_MATH_HW_EXP2 = 7,
  SMC_TEST_MATH_HW_LOG = 8,
  SMC_TEST_MATH_M2LOG_U32 = 9,
  SMC_TEST_MATH_SQRT_RADIUS = 10,
  SMC_TEST_MATH_SINCOS_U32 = 11,
  SMC_TEST_MATH_EXP2S = 12,
  SMC_TEST_MATH_MUL_EXP2S = 13,
  SMC_TEST_MATH_NORMAL_F64 = 14,
  SMC_TEST_MATH_TWIDDLE = 15,
  SMC_TEST_MATH_COUNT = 16
};
int32_t smc_test_math_eval(int32_t fn, const void* in_dev, int64_t n, void* out_dev, void* stream);

/* The host plan of smc_gbm_greeks_paths for a shape (tests/test_path_greeks_host.py; no device call): *sweep_rows is R,
 * the accumulator row pairs of a NORMALIZE sweep (0 under RAW), *lds_bytes the dynamic LDS of the launch.
 * SMC_ERR_INVALID_ARGUMENT: hooks disabled, NULL pointer; SMC_ERR_INVALID_SHAPE: timesteps <= 0 or a shape, scheme or
 * dtype path_greeks_kernel does not take. */
int32_t smc_test_path_greeks_plan(int32_t timesteps, int32_t scheme, int32_t normalization, int32_t dtype,
                                  int64_t* sweep_rows, int64_t* lds_bytes);

#ifdef __cplusplus
}
#endif

#endif /* SPECTRALMC_HIP_TESTING_H */
