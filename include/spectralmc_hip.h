/*
 * spectralmc_hip.h — C ABI of the MI355X (gfx950) GbmCVNNPricer hot path.
 *
 * One shared library, libspectralmc_hip.so, exports these symbols with plain
 * pointers and sizes (no torch / HIP C++ types in the signatures).  Every entry
 * point is stream-ordered on the caller's `hipStream_t` (passed as `void*`,
 * NULL = legacy default stream), allocates nothing per call, performs no host
 * synchronisation and no hidden H2D/D2H copy, so a caller may capture any
 * sequence of these calls into a hipGraph.  All device buffers are caller-owned.
 *
 * Reference seams replaced (Tuee22/SpectralMC @ 2026-01-02, paths relative to
 * the reference repository root):
 *   smc_sobol_*          scipy.stats.qmc.Sobol(d, scramble=True, seed) + fast_forward + random,
 *                        as used by SobolSampler.create / sample
 *                        (src/spectralmc/sobol_sampler.py:177-203, 222-246)
 *   smc_gbm_simulate     ConcurrentNormGenerator.get_matrix + SimulateBlackScholes[grid, tpb, stream]
 *                        (src/spectralmc/async_normals.py:388-398, src/spectralmc/gbm.py:224-257, 400-426)
 *   smc_gbm_normalize    forward normalisation sims *= forwards / row_means
 *                        (src/spectralmc/gbm.py:428-440)
 *   smc_cf_targets       put payoff + reshape(M, N) + FFT(axis=1) + mean(axis=0)
 *                        (src/spectralmc/gbm.py:464-474, src/spectralmc/gbm_trainer.py:806-817)
 *   smc_train_targets    the fused per-step Monte-Carlo side of _run_batch: all of the above for
 *                        B contracts in one launch sequence (src/spectralmc/gbm_trainer.py:1546-1556)
 *   smc_normals          the normal matrix the engine consumes for contract ordinal m
 *                        (async_normals.py:212-216 stream semantics; values are this library's RNG)
 *
 * Status codes are mapped to the reference's error dataclasses by the Python
 * host layer (spectralmc_amd/_lib.py); smc_last_error_string() gives the text of
 * the last failure on the calling thread.
 */
#ifndef SPECTRALMC_HIP_H
#define SPECTRALMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMC_ABI_VERSION 21  /* 16: smc_gbm_price; 17: smc_gbm_price_paths; 18: smc_basket_price; 19: smc_gbm_greeks; 20: smc_basket_greeks; 21: smc_basket_price_general; smc_basket_greeks_general (with its _kernel and _cols queries) was added under 21 without a new number: the change is purely additive, no existing entry point moved, and the library ships together with the bindings that load it; smc_basket_price_paths (with its _kernel query) was added under 21 in the same way, so was smc_gbm_price_sliced (with its _workspace_bytes and _kernel queries and smc_gbm_price_slice_paths), and so was smc_gbm_greeks_paths (with its _kernel query) */

/* ---- status codes ------------------------------------------------------- */
#define SMC_OK                      0
#define SMC_ERR_INVALID_ARGUMENT    1  /* null pointer, bad enum, dim out of range    */
#define SMC_ERR_INVALID_SHAPE       2  /* sizes the kernels cannot take (e.g. N>4096)  */
#define SMC_ERR_SEED_OUT_OF_RANGE   3  /* seed/skip outside what the engine accepts    */
#define SMC_ERR_SEQUENCE_EXHAUSTED  4  /* Sobol index would pass 2^30 points           */
#define SMC_ERR_MEMORY_LIMIT        5  /* reference gbm.py:106-137 path-count guard     */
#define SMC_ERR_HIP                 6  /* HIP runtime error (launch / device)           */
#define SMC_ERR_EXCHANGE_TIMEOUT    7  /* a co-resident partner workgroup never arrived
                                          (smc_sync_status; NaN targets were written)     */

/* ---- enums (values mirror the reference enums' order) ------------------- */
#define SMC_SCHEME_LOG_EULER     0  /* PathScheme.LOG_EULER   effects/montecarlo.py:24-29 */
#define SMC_SCHEME_SIMPLE_EULER  1  /* PathScheme.SIMPLE_EULER                           */
#define SMC_NORM_RAW             0  /* ForwardNormalization.RAW  effects/montecarlo.py:30-35 */
#define SMC_NORM_NORMALIZE       1  /* ForwardNormalization.NORMALIZE                    */
#define SMC_DTYPE_F32            0  /* Precision.float32 (paths f32, targets complex64)  */
#define SMC_DTYPE_F64            1  /* Precision.float64 (paths f64, targets complex128) */
#define SMC_MATH_HW          0x100  /* flag, OR into `scheme` (engine calls) or `dtype` (smc_normals):
                                      f32 hardware transcendentals (v_exp/v_log/v_sin/v_cos/v_sqrt)
                                      instead of the portable, CPU-reproducible kernels */
#define SMC_MATH_REF         0x400  /* flag, OR into smc_train_targets' / smc_train_step's `scheme` (f32
                                      only): the reference kernel's own typing (gbm.py:224-257 under
                                      Numba: f64 state and step of the f32 normals, f32 stores): portable
                                      normals, the f64 engine's step, rounded f32 paths (rows_ref_kernel +
                                      cf_kernel).  The f64 step's exp is within 2 ulp of libm's, so a
                                      stored f32 value equals the reference arithmetic's except where the
                                      two exps round to different floats (C2 shape: <= 1e-6 of the values,
                                      1 ulp; tests/test_oracle.py).  With SMC_MATH_HW (ABI 15): the same
                                      step on the hardware-transcendental f32 normals (within 1.1e-6 of
                                      the exact ones, so not bit-reproducible on a CPU).  In the kernel
                                      queries' dtype: that kernel's name */
#define SMC_TRAIN_DYNAMIC    0x200  /* flag, OR into smc_train_step's `scheme`: the whole-contract resident
                                      launch hands out every contract from its contract queue (default:
                                      the first three quarters of the rounds statically), for launches that
                                      may start while the previous step's launch still holds CUs */
#define SMC_STORE_TERMINAL       1  /* keep only the terminal row [B][P] (scratch)        */
#define SMC_STORE_ALL            2  /* materialise the full path matrix [B][T][P]         */

#define SMC_SOBOL_BITS 30           /* scipy Sobol bits=30: at most 2^30 points          */

typedef struct smc_sobol smc_sobol;

int32_t     smc_abi_version(void);
const char* smc_last_error_string(void);
/* Kernel timing for measurement (ABI 14): arms two caller-created hipEvent_t for the engine calls that
 * follow on this thread (smc_train_step, smc_train_targets, smc_basket_train_targets): their first path /
 * CF kernel records start_event at its own start, every path / CF kernel records stop_event at its own
 * end (hipExtLaunchKernel), so after the call the pair spans the call's path and CF kernels as a kernel
 * trace times them, without the dispatch gaps of stream events around back-to-back launches.  The
 * auxiliary kernels (Sobol draw, cursor update, normalisation, normals) are not timed.  NULL, NULL
 * disarms.  Stream-ordered like the launches; captured launches record nothing. */
int32_t     smc_time_launches(void* start_event, void* stop_event);

/* ---- sync-area status (smc_train_step, smc_basket_train_targets) ---------- */
/* Launches whose workgroups exchange sums (the sliced resident kernel, the resident basket kernel)
 * poll for their partners a bounded time (~1 s).  A partner that never arrives (e.g. the group's
 * workgroups were not all co-resident) sets SMC_SYNC_EXCHANGE_TIMEOUT in the 32-bit status word at
 * byte SMC_SYNC_STATUS_OFFSET of the sync area and the launch's own failure flag (byte
 * SMC_SYNC_LAUNCH_FAIL_OFFSET); the launch still completes (every later wait of THAT launch sees its
 * flag and gives up at once) with NaN targets for the contracts it could not finish.  The last
 * workgroup of the launch clears the flag, so the next launch waits normally; the status word is
 * sticky across launches: the caller reads (and clears) it with smc_sync_status. */
#define SMC_SYNC_STATUS_OFFSET     32
#define SMC_SYNC_LAUNCH_FAIL_OFFSET 48
#define SMC_SYNC_EXCHANGE_TIMEOUT  1u
/* Waits for `stream`, then copies the status word of sync_dev to *status_out (0: no failure) and,
 * if clear != 0, zeroes it.  The only call of this ABI that synchronises the host. */
int32_t smc_sync_status(void* sync_dev, int32_t clear, int32_t* status_out, void* stream);
/* ---- scrambled Sobol (SciPy-bit-exact) ---------------------------------- */
/* Build the LMS+digital-shift scrambled generator SciPy builds for
 * Sobol(d=dim, scramble=True, seed=seed), then fast_forward(skip).
 * dim in [1, 64]; seed in [0, 2^63). */
int32_t smc_sobol_create(int32_t dim, uint64_t seed, uint64_t skip, smc_sobol** out);
void    smc_sobol_destroy(smc_sobol* h);
/* Host copies of the scrambled tables and the host cursor (next point index). */
int32_t smc_sobol_state(const smc_sobol* h, uint32_t* shift /*[dim]*/, uint32_t* sv /*[dim*30]*/,
                        uint64_t* cursor);
int32_t smc_sobol_fast_forward(smc_sobol* h, uint64_t n);
/* Host draw of n raw points in [0,1) (Sobol.random(n)); advances the host cursor. */
int32_t smc_sobol_random_host(smc_sobol* h, int64_t n, double* out /*[n][dim] host*/);
/* Table image for the device draw: tables[0..dim) = shift, tables[dim + d*30 + c] = sv[d][c].
 * The caller copies it into a device buffer of dim*31 u32 it owns. */
int32_t smc_sobol_export_tables(const smc_sobol* h, uint32_t* tables /*[dim*31] host*/);
/* Device draw from an uploaded table image: point i of the batch is sequence index
 *   (*index_dev if index_dev != NULL else 0) + index0 + i
 * scaled as lower + (upper - lower) * x in f64 exactly as sobol_sampler.py:239.
 * out_f64: [n][dim] f64 (required); out_f32: [n][dim] f32 copy or NULL (CVNN input,
 * gbm_trainer.py:1775-1783).  The caller guarantees the index range stays < 2^30. */
int32_t smc_sobol_draw(const uint32_t* tables_dev, int32_t dim, const int64_t* index_dev,
                       int64_t index0, int64_t n, const double* lower_dev, const double* upper_dev,
                       double* out_f64, float* out_f32, void* stream);

/* ---- GBM Monte-Carlo engine --------------------------------------------- */
/* contracts_dev: [B][6] f64 rows in BlackScholes.Inputs order X0, K, T, r, d, v.
 * Contract b uses normal stream ordinal (*ordinal_dev if non-NULL else 0) + ordinal0 + b.
 * paths_dev: [B][T][P] of the dtype (raw, un-normalised paths; row t = value after step t+1).
 * rowsum_dev: [B][T] f64 sums over the P paths of each row (may be NULL). */
int32_t smc_gbm_simulate(const double* contracts_dev, int64_t n_contracts, int32_t timesteps,
                         int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                         int64_t ordinal0, int32_t scheme, int32_t dtype,
                         void* paths_dev, double* rowsum_dev, void* stream);
/* In-place forward normalisation of a [B][T][P] path matrix from its row sums. */
int32_t smc_gbm_normalize(const double* contracts_dev, int64_t n_contracts, int32_t timesteps,
                          int64_t n_paths, int32_t dtype, void* paths_dev,
                          const double* rowsum_dev, void* stream);
/* CF targets from a stored raw path matrix ([B][T][P], row T-1 is read) and its
 * row sums: targets[b][k] = FFT_N(mean_M(put.reshape(M, N)))[k], N*M == P. */
int32_t smc_cf_targets(const double* contracts_dev, int64_t n_contracts, int32_t timesteps,
                       int32_t network_size, int32_t batches_per_mc_run, int32_t normalization,
                       int32_t dtype, const void* paths_dev, const double* rowsum_dev,
                       void* targets_dev, void* stream);
/* Fused training targets: simulate + (store) + normalise + payoff + M-mean + DFT for
 * B contracts.  store_mode SMC_STORE_ALL writes the full matrix into paths_dev, which
 * holds `chunk_contracts` contracts ([chunk][T][pitch]) and is reused chunk by chunk;
 * SMC_STORE_TERMINAL needs paths_dev of [chunk][pitch].  path_pitch: elements between
 * consecutive path rows (0 = P, contiguous; else a multiple of 4 >= P, e.g. smc_path_pitch).
 * targets_dev: [B][N] complex.
 * workspace_dev (may be NULL): smc_engine_workspace_bytes(chunk, T, P, rowsum_dev != NULL)
 * bytes, zero-filled once before first use (the kernel leaves it zeroed).  With a workspace
 * each contract is simulated by several workgroups (slices of 8192 paths) and the last one
 * to finish runs the payoff/DFT phase; without it one workgroup runs the whole contract.
 * Results are bit-identical run to run either way; the two differ only in the f64 row-sum
 * association (oracle/gbm_oracle.c restates both). */
int32_t smc_train_targets(const double* contracts_dev, int64_t n_contracts, int32_t timesteps,
                          int32_t network_size, int32_t batches_per_mc_run, uint64_t mc_seed,
                          const int64_t* ordinal_dev, int64_t ordinal0, int32_t scheme,
                          int32_t normalization, int32_t dtype, int32_t store_mode,
                          void* paths_dev, int64_t path_pitch, int64_t chunk_contracts,
                          double* rowsum_dev, void* targets_dev, void* workspace_dev,
                          int64_t workspace_bytes, void* stream);
/* One Monte-Carlo step of the training loop (sobol_sampler.py:222-246 + gbm_trainer.py:1546-1556):
 * the Sobol draw of the step's contracts (point i = sequence index cursor_dev[0] + index_offset + i,
 * scaled as smc_sobol_draw, into contracts_dev [B][6] f64 and cvnn_input_dev [B][6] f32 or NULL),
 * the targets with ordinal_dev = cursor_dev + 1, ordinal0 = index_offset, then
 * cursor_dev[0..1] += advance.  Where the resident kernel takes the shape (f32, T = 16, P a
 * multiple of 4096 up to 8 x 65,536, N | 4096) each chunk of contracts is ONE launch: each
 * workgroup draws the rows of its own contracts and the last workgroup of the last chunk advances
 * the cursor.  P <= 65,536: one workgroup per contract, targets bit-identical to
 * smc_sobol_draw + smc_train_targets (no workspace) + the cursor update.  P > 65,536 (C3): W =
 * P / 65,536 co-resident workgroups per contract exchange their terminal and column sums through
 * the sync area; the f64 sums are added in slice order (oracle kernel mode, slices = W).  Other
 * shapes run the three steps as separate launches, bit-identical to the separate calls.
 * sync_dev: smc_train_step_sync_bytes(...) bytes, zero-filled before the first call (every call
 * leaves its counters zeroed; the status word at SMC_SYNC_STATUS_OFFSET is sticky, see
 * smc_sync_status). */
int32_t smc_train_step(const uint32_t* sobol_tables_dev, int32_t dim, const double* lower_dev,
                       const double* upper_dev, int64_t* cursor_dev, int64_t index_offset, int64_t advance,
                       double* contracts_dev, float* cvnn_input_dev, int64_t n_contracts, int32_t timesteps,
                       int32_t network_size, int32_t batches_per_mc_run, uint64_t mc_seed, int32_t scheme,
                       int32_t normalization, int32_t dtype, int32_t store_mode, void* paths_dev,
                       int64_t path_pitch, int64_t chunk_contracts, void* targets_dev, void* sync_dev,
                       int64_t sync_bytes, void* stream);
/* Bytes of smc_train_step's sync area for this shape on the current device (128 for whole-contract
 * shapes: a done counter, the status word and the contract queue: the resident kernel's dynamically
 * handed-out last quarter of the rounds, rows_kernel's contracts after each workgroup's first; -1 if
 * the device query fails). */
int64_t smc_train_step_sync_bytes(int32_t timesteps, int32_t network_size, int32_t batches_per_mc_run,
                                  int32_t dtype, int64_t path_pitch);
/* Name of the kernel smc_train_step launches for this shape ("resident_kernel",
 * "resident_kernel(sliced)", or smc_train_targets_kernel's name).  Static string.  dtype may carry
 * SMC_QUERY_RAW: the shape's targets use RAW normalisation (one-wave-per-contract shapes); a bit of its
 * own (ABI 12: it was 0x100, SMC_MATH_HW's bit in smc_normals' dtype); and SMC_MATH_REF (ABI 13). */
#define SMC_QUERY_RAW 0x1000
const char* smc_train_step_kernel(int32_t timesteps, int32_t network_size, int32_t batches_per_mc_run,
                                  int32_t dtype, int64_t path_pitch);
/* Workspace bytes smc_train_targets needs for sliced contracts (0: P too small to slice). */
int64_t smc_engine_workspace_bytes(int64_t chunk_contracts, int32_t timesteps, int64_t n_paths,
                                   int32_t all_rows);
/* Name of the kernel smc_train_targets launches for this shape ("wave_kernel", "resident_kernel",
 * "packed_kernel", the split pairs, "contract_kernel", "queue_kernel" or "rows_ref_kernel+cf_kernel";
 * sliced = a workspace is passed; dtype | SMC_QUERY_RAW | SMC_MATH_REF as for smc_train_step_kernel;
 * "unsupported" for an SMC_MATH_REF shape the engine rejects: f64, a pitch without room for the terminal
 * sum, sliced).  Static string. */
const char* smc_train_targets_kernel(int32_t timesteps, int32_t network_size, int64_t n_paths,
                                     int32_t dtype, int64_t path_pitch, int32_t sliced);
/* Recommended row pitch (elements) for a path scratch buffer of n_paths columns: the row
 * stride becomes an odd multiple of 4 KiB (power-of-two strides alias in HBM). */
int64_t smc_path_pitch(int64_t n_paths, int32_t dtype);
/* The [rows][cols] N(0,1) matrix of contract ordinal m (the values smc_gbm_simulate
 * draws for path p, step t, laid out [t][p]; rows = the contract's T: at T <= 2 one
 * Philox-seeded stream serves 4 consecutive 4-path groups, the stream span of smc_rng.h). */
int32_t smc_normals(uint64_t mc_seed, int64_t ordinal, int32_t rows, int64_t cols,
                    int32_t dtype, void* out_dev, void* stream);

/* ---- correlated multi-asset (basket) engine ---------------------------------
 * Extension of the reference engine (BASELINE.json configs[4]; per-asset dynamics as
 * SimulateBlackScholes, src/spectralmc/gbm.py:224-257, log-Euler; normalisation gbm.py:428-440;
 * targets as _simulate_fft, gbm_trainer.py:806-817) with an equal-weight basket put.
 * contracts_dev: [B][3A+4] f64 rows (K, T, r, rho, X0[A], d[A], v[A]); the equicorrelation
 * matrix (1-rho) I + rho 11^T is Cholesky-factored in LDS per contract.
 * paths_dev: [chunk][A][T][pitch] f32 (SMC_STORE_ALL) or [chunk][A][pitch] (SMC_STORE_TERMINAL),
 * reused per launch of chunk_contracts; terminal_sum_dev (may be NULL): [B][A] f64 sums of the
 * terminal rows; targets_dev: [B][N] complex64.  math: 0 (portable, CPU-reproducible) or
 * SMC_MATH_HW.  Needs 1 <= A <= 8, N % 4 == 0, N <= 4096, N*M a multiple of 2048.
 * sync_dev (may be NULL): smc_basket_sync_bytes(...) bytes, zero-filled before the first call (every
 * call leaves its counters zeroed).  With it, shapes the resident kernel takes (T = 16, N | 4096, N <= 2048,
 * N*M a multiple of 4096 up to 32 x 4096) run basket_resident_kernel per chunk, in which W = N*M /
 * 4096 co-resident workgroups per contract keep the terminal rows on chip and exchange their
 * terminal sums, then basket_mean_fft_kernel over the slices' column sums (reduction orders:
 * oracle_basket_kernel(wg = 1024, slices = W)).  Otherwise, with
 * terminal_sum_dev each chunk is two launches (simulate + store + terminal sums, then the CF pass
 * over the stored terminal rows), without it one fused launch; these two are bit-identical. */
int32_t smc_basket_train_targets(const double* contracts_dev, int64_t n_contracts, int32_t n_assets,
                                 int32_t timesteps, int32_t network_size, int32_t batches_per_mc_run,
                                 uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0,
                                 int32_t math, int32_t normalization, int32_t store_mode,
                                 void* paths_dev, int64_t path_pitch, int64_t chunk_contracts,
                                 double* terminal_sum_dev, void* targets_dev, void* sync_dev,
                                 int64_t sync_bytes, void* stream);
/* Bytes of smc_basket_train_targets' sync area for this shape and chunk_contracts on the current
 * device (slice-sum exchange + the column sums of one launch; 0: the resident kernel does not take
 * the shape, pass NULL; -1 on a bad argument or a failed query). */
int64_t smc_basket_sync_bytes(int32_t n_assets, int32_t timesteps, int32_t network_size,
                              int32_t batches_per_mc_run, int64_t chunk_contracts);
/* Name of the kernel(s) smc_basket_train_targets launches for this shape ("basket_resident_kernel",
 * "basket_kernel+basket_cf_kernel" or "basket_kernel"); with_sync / keep_sums: whether the call
 * passes sync_dev / terminal_sum_dev.  Static string. */
const char* smc_basket_train_targets_kernel(int32_t n_assets, int32_t timesteps, int32_t network_size,
                                            int32_t batches_per_mc_run, int32_t with_sync, int32_t keep_sums);
/* Basket workgroups (one per contract) resident on the current device at once, for sizing
 * chunk_contracts in whole rounds; -1 on a bad argument or a failed device query. */
int64_t smc_basket_resident_slots(int32_t n_assets, int32_t network_size, int32_t math);

/* ---- complex-valued MLP training step --------------------------------------
 * Replaces the network half of _torch_step (src/spectralmc/gbm_trainer.py:819-835) for
 * ComplexSequential chains of ComplexLinear (cvnn.py:65-143) with optional modReLU
 * (cvnn.py:168-210) or zReLU (cvnn.py:149-162) activations.  Parameters, gradients and Adam
 * moments are flat buffers in the model's parameter order; a layer names its tensors by
 * element offset into them (-1 = absent). */
#define SMC_CVNN_MAX_LAYERS 8
#define SMC_ACT_NONE     0
#define SMC_ACT_MODRELU  1
#define SMC_ACT_ZRELU    2

typedef struct smc_cvnn_layer {
  int32_t in_features, out_features;
  int32_t activation;            /* SMC_ACT_* applied after this layer's affine map */
  int32_t reserved;
  int64_t w_re, w_im;            /* [out][in] real_weight / imag_weight offsets        */
  int64_t b_re, b_im;            /* [out] real_bias / imag_bias offsets or -1          */
  int64_t act_bias;              /* [out] modReLU bias offset or -1                    */
} smc_cvnn_layer;

/* Where an Adam update also writes the matrix-core (MFMA) operand copies of the weights it changes, so the
 * next smc_cvnn_mfma_forward_backward skips its pack launch (mode | SMC_CVNN_MFMA_PACKED): each complex
 * weight w = a + i b of layer l lands at Wc[2j][2k] = Wc[2j+1][2k+1] = a, Wc[2j][2k+1] = -b, Wc[2j+1][2k] = b
 * and at the same places of Wc^T (smc_cvnn_mfma_pack_plan fills it from the forward_backward plan). */
typedef struct smc_cvnn_pack_layer {
  int64_t w_re, w_im;            /* the layer's weight offsets in params (as smc_cvnn_layer)   */
  int32_t ni, no;                /* complex in / out features                                  */
  int32_t win, wout;             /* packed widths (2 ni, 2 no rounded up to the K block)       */
  int64_t wc, wct;               /* element offsets of Wc [wout][win] and Wc^T [win][wout]     */
} smc_cvnn_pack_layer;
typedef struct smc_cvnn_pack {
  void* ws;                      /* the forward_backward workspace                             */
  int32_t bf16;                  /* operands are bf16 (SMC_CVNN_MFMA_BF16), else f32           */
  int32_t n_layers;              /* 0: nothing to write                                        */
  smc_cvnn_pack_layer layer[SMC_CVNN_MAX_LAYERS];
} smc_cvnn_pack;

/* torch.optim.Adam (defaults of gbm_trainer.py:1513) on flat buffers; `step` is torch's
 * capturable f32 step counter, read before and incremented after the update. */
typedef struct smc_adam_args {
  void* params;
  void* exp_avg;
  void* exp_avg_sq;
  float* step;
  double lr, beta1, beta2, eps, weight_decay;
  double* norm_partials;         /* [smc_adam_norm_partials(n_params)] scratch, ZEROED before
                                    the first call (its last slot is the fused finalize's
                                    arrival counter; every COMPLETED call leaves it zero:
                                    a caller that allocates it without zeroing, or reuses
                                    it after a launch that did not complete, must zero it
                                    again, else no workgroup counts as last and grad_norm,
                                    loss and step stop being written)                      */
  void* grad_norm;               /* scalar out: ||grad||_2 (gbm_trainer.py:834)         */
  void* loss;                    /* scalar out: grads[n_params] (the loss slot)         */
  const smc_cvnn_pack* pack;     /* or NULL: the update also writes these packed copies (ABI 13) */
} smc_adam_args;

/* Number of per-workgroup gradient partials ([blocks][n_params + 1]) for this batch. */
int32_t smc_cvnn_plan(const smc_cvnn_layer* layers, int32_t n_layers, int32_t dtype, int64_t batch,
                      int64_t* partial_blocks);
/* Forward, loss = mse(Re) + mse(Im), backward: partials[g] = the gradients and loss share
 * of workgroup g's rows.  input_im may be NULL (zeros); targets [batch][N] complex. */
int32_t smc_cvnn_forward_backward(const smc_cvnn_layer* layers, int32_t n_layers, int32_t dtype,
                                  const void* params, int64_t n_params, const void* input_re,
                                  const void* input_im, const void* targets, int64_t batch,
                                  void* partials, int64_t partial_blocks, void* stream);
/* grads[0..n_params] = fixed-order sum of the partials (last entry: loss).  With adam != NULL
 * the Adam update, grad norm, loss copy and step increment follow (ABI 12: for networks of up to
 * 65,535 parameters in the same launch, whose last workgroup takes the grad norm, loss and step;
 * larger ones in a second, one-workgroup launch). */
int32_t smc_cvnn_reduce_grads(int32_t dtype, const void* partials, int64_t partial_blocks,
                              int64_t n_params, void* grads, const smc_adam_args* adam, void* stream);
/* Adam update from an already reduced (e.g. all-reduced) grads[0..n_params]. */
int32_t smc_adam_step(int32_t dtype, int64_t n_params, const void* grads, const smc_adam_args* adam,
                      void* stream);
/* f64 entries of smc_adam_args.norm_partials: one per 64 gradient entries + the arrival counter. */
int64_t smc_adam_norm_partials(int64_t n_params);

/* ---- the same network step on the matrix cores (csrc/cvnn_mfma.hip) ---------
 * Each complex layer runs as real GEMMs of the interleaved (re, im) vectors on MFMA:
 *   SMC_CVNN_MFMA_F32   f32 operands (v_mfma_f32_16x16x4_f32), the network's own precision;
 *   SMC_CVNN_MFMA_BF16  bf16 operands rounded to nearest even, f32 accumulation, f32 master
 *                       parameters / activations / loss / Adam (BASELINE configs[2] "bf16 CVNN";
 *                       an extension: the reference asserts full precision, gbm_trainer.py:679-686).
 * Parameters, inputs and targets are f32 / complex64.  The call writes per-segment partials
 * [partial_blocks][n_params + 1] (gradients, loss last) that smc_cvnn_reduce_grads(SMC_DTYPE_F32,
 * ...) sums in order, exactly as after smc_cvnn_forward_backward.  Shapes whose widths exceed the
 * kernels' LDS plan return SMC_ERR_INVALID_SHAPE from the plan (callers keep the VALU kernels). */
#define SMC_CVNN_MFMA_F32   1
#define SMC_CVNN_MFMA_BF16  2
#define SMC_CVNN_MFMA_PACKED 0x100  /* flag, OR into forward_backward's mode: the workspace already holds
                                       the packed weights of params (the last Adam update wrote them).
                                       Valid only while params change through those updates alone: a
                                       caller that writes params any other way (a state_dict load, a
                                       broadcast) must drop the flag for the next call (net.py
                                       FusedNetworkStep.invalidate_pack) */
int32_t smc_cvnn_mfma_plan(const smc_cvnn_layer* layers, int32_t n_layers, int32_t mode, int64_t batch,
                           int64_t* partial_blocks, int64_t* workspace_bytes);
int32_t smc_cvnn_mfma_forward_backward(const smc_cvnn_layer* layers, int32_t n_layers, int32_t mode,
                                       const float* params, int64_t n_params, const float* input_re,
                                       const float* input_im, const void* targets, int64_t batch,
                                       float* partials, int64_t partial_blocks, void* workspace,
                                       int64_t workspace_bytes, void* stream);
/* The packed-weight layout of that plan for Adam (smc_adam_args.pack); out->n_layers = 0 for plans whose
 * wide layers keep their own pack launch (the layered GEMM path). */
int32_t smc_cvnn_mfma_pack_plan(const smc_cvnn_layer* layers, int32_t n_layers, int32_t mode, int64_t batch,
                                void* workspace, smc_cvnn_pack* out);

/* ---- batched Monte-Carlo pricing (ABI 16) -----------------------------------
 * BlackScholes.price + get_host_price (src/spectralmc/gbm.py:442-497) for B contracts in ONE launch:
 * one workgroup per contract simulates the P paths in the simulate call's order (same streams: contract b
 * uses ordinal (*ordinal_dev or 0) + ordinal0 + b) and writes no path row: the terminal values stay on
 * chip and leave as SMC_PRICE_COLS doubles per contract, prices_dev [B][8]:
 *   0 put price, 1 call price, 2 underlying (means over the P paths of df max(K - xs, 0),
 *   df max(xs - K, 0) and xs, each evaluated in the sim dtype as the CF targets' payoff is and added in f64;
 *   xs = x F / mean(x) under SMC_NORM_NORMALIZE, x under SMC_NORM_RAW),
 *   3 put / 4 call standard error of that mean (0 at P = 1), 5 put / 6 call intrinsic value
 *   df max(K - F, 0) / df max(F - K, 0), 7 the f64 sum of the raw terminal values.
 * Every sum has one fixed order: the block is bit-identical run to run, under any split of the batch and
 * whichever way the kernel keeps the terminal values (NORMALIZE needs them twice: parked in LDS for
 * contracts of up to 144 KiB of terminal values, else simulated a second time; SMC_PRICE_REPLAY forces the
 * latter).  scheme takes SMC_MATH_HW (f32 only); SMC_MATH_REF is rejected.  B below the CU count leaves
 * CUs idle (a contract is not split over workgroups). */
#define SMC_PRICE_COLS   8
#define SMC_PRICE_REPLAY 0x800   /* flag, OR into the price call's scheme: never park in LDS */
int32_t smc_gbm_price(const double* contracts_dev, int64_t n_contracts, int32_t timesteps, int64_t n_paths,
                      uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t scheme,
                      int32_t normalization, int32_t dtype, double* prices_dev /*[B][8]*/, void* stream);
/* Name of the kernel that call launches for this shape: "price_kernel(raw)", "price_kernel(lds)",
 * "price_kernel(replay)", or "unsupported".  Static string, no device call. */
const char* smc_gbm_price_kernel(int32_t timesteps, int64_t n_paths, int32_t scheme, int32_t normalization,
                                 int32_t dtype);

/* ---- path-dependent batched pricing (ABI 17) --------------------------------
 * Average-price (Asian), knock-out and fixed-strike lookback options beside the European pair, for B
 * contracts in ONE launch and without a path matrix in memory: one workgroup per contract with the price
 * call's streams, geometry and fixed sum order, so the block is bit-identical run to run and under any
 * split of the batch.  The monitoring dates are the T grid points of the simulate call's matrix (X0 itself
 * is not monitored).  Row t is seen as xs_t = x_t s_t rounded to the sim dtype: s_t = F_t / mean_p(x_t) under
 * SMC_NORM_NORMALIZE (bit for bit the rows the simulate + normalize calls leave in memory, in portable
 * math), xs_t = x_t under SMC_NORM_RAW.  Per path, in the sim dtype: avg = (sum_t xs_t) / T, mx = max_t xs_t,
 * mn = min_t xs_t, ko = any_t (xs_t <= lower || xs_t >= upper); each payoff is df max(. , 0) in the sim dtype,
 * cast to f64 and averaged over the P paths.  prices_dev [B][20]:
 *    0 Asian put  (K - avg)            1 Asian call  (avg - K)
 *    2 knock-out put (0 if ko, else K - xs_T)   3 knock-out call (0 if ko, else xs_T - K)
 *    4 lookback put (K - mn)           5 lookback call (mx - K)
 *    6 European put (K - xs_T)         7 European call (xs_T - K): the price call's columns 0 and 1
 *    8..15 the standard errors of columns 0..7 (0 at P = 1)
 *   16 mean of avg, 17 knocked share (count / P), 18 mean of mx, 19 mean of mn.
 * barriers_dev [B][2] holds (lower, upper) per contract; NULL means no barrier (columns 2, 3 equal 6, 7 and
 * column 17 is 0); a lower <= 0 or an upper of +inf switches that side off.  A knock-in is the European
 * column minus the knock-out column.  RAW is one pass; NORMALIZE simulates twice (row sums, then payoffs;
 * more often when T exceeds the 26 to 34 rows of per-lane f64 accumulators that fit in LDS).  scheme takes
 * SMC_MATH_HW (f32 only); SMC_MATH_REF, SMC_TRAIN_DYNAMIC and SMC_PRICE_REPLAY are rejected, and so is
 * (SMC_ERR_INVALID_SHAPE) a NORMALIZE run of more time steps than LDS holds row scales for (about 34,000
 * in f32, 12,800 in f64).  Monitoring is discrete: no continuity correction; arithmetic averages only. */
#define SMC_PATH_PRICE_COLS 20
int32_t smc_gbm_price_paths(const double* contracts_dev /*[B][6]*/, const double* barriers_dev /*[B][2] or NULL*/,
                            int64_t n_contracts, int32_t timesteps, int64_t n_paths, uint64_t mc_seed,
                            const int64_t* ordinal_dev, int64_t ordinal0, int32_t scheme, int32_t normalization,
                            int32_t dtype, double* prices_dev /*[B][20]*/, void* stream);
/* "path_price_kernel(raw)", "path_price_kernel(replay)" or "unsupported".  Static string, no device call. */
const char* smc_gbm_price_paths_kernel(int32_t timesteps, int64_t n_paths, int32_t scheme, int32_t normalization,
                                       int32_t dtype);

/* ---- batched basket pricing (ABI 18) ------------------------------------------
 * Monte-Carlo prices of the equal-weight basket and of the two rainbow payoffs (best-of, worst-of) on the
 * correlated multi-asset engine, for B contracts in ONE launch and without a terminal buffer in memory: one
 * workgroup per contract with smc_basket_train_targets' contract rows ([B][3A+4]: K, T, r, rho, X0[A], d[A],
 * v[A]), streams (contract b uses ordinal (*ordinal_dev or 0) + ordinal0 + b), Cholesky and packed f32 step;
 * the A terminal values of a path stay in registers.  Unlike the training call any n_paths >= 1 is taken.
 * Per path, all in f32 (the engine's only dtype; the training targets' payoff arithmetic):
 *   xs_i = x_i s_i, s_i = F_i / f32(tot_i / P) under SMC_NORM_NORMALIZE (F_i = f32(X0_i) exp(f32(r - d_i) f32(T)),
 *   tot_i the f64 sum of asset i's raw terminal values), s_i = 1 under SMC_NORM_RAW;
 *   bk = (((0 + xs_0) + xs_1) + ...) f32(1 / A), mx = max_i xs_i, mn = min_i xs_i;
 *   each payoff is df max(. , 0) with df = exp(f32(-r) f32(T)), cast to f64 and averaged over the P paths.
 * prices_dev [B][18]:
 *    0 basket put    (K - bk)            1 basket call    (bk - K)
 *    2 best-of put   (K - mx)            3 best-of call   (mx - K)
 *    4 worst-of put  (K - mn)            5 worst-of call  (mn - K)
 *    6..11 the standard errors of columns 0..5 (0 at P = 1)
 *   12 mean of bk, 13 mean of mx, 14 mean of mn, 15 exercise share of the basket put (count(bk < K) / P)
 *   16 / 17 intrinsic basket put / call df max(K - Fb, 0) / df max(Fb - K, 0), Fb = (((0 + F_0) + F_1) + ...) f32(1 / A).
 * terminal_sum_dev (may be NULL): [B][A] f64, the tot_i (smc_basket_train_targets' terminal sums bit for bit
 * where n_paths is a multiple of 2048).  Every sum has one fixed order: the block is bit-identical run to run,
 * under any split of the batch and whichever way the kernel keeps the terminal values (NORMALIZE needs them
 * twice: parked in LDS while A * roundup4(P) * 4 bytes and 2112 bytes of scratch fit in 144 KiB, else simulated
 * a second time; SMC_PRICE_REPLAY forces the latter).  math: 0 (portable, CPU-reproducible) or SMC_MATH_HW,
 * optionally | SMC_PRICE_REPLAY; any other bit (SMC_MATH_REF, SMC_TRAIN_DYNAMIC, ...) is rejected.
 * SMC_ERR_INVALID_ARGUMENT: NULL contracts_dev / prices_dev, n_assets outside 1..8, bad math, bad
 * normalization.  SMC_ERR_INVALID_SHAPE: n_contracts < 0 or >= 2^31, timesteps <= 0, n_paths <= 0 or >= 2^40.
 * All of these are reported before the empty batch (n_contracts = 0: SMC_OK, nothing touched) is accepted.
 * Contract values are not validated on the device, as in the engine: an indefinite correlation matrix
 * (rho <= -1 / (A - 1)) gives NaN, and rho = 1 is only meaningful for A <= 2 (from A = 3 on the
 * Banachiewicz factorisation divides 0 by 0).  B below the CU count leaves CUs idle (a contract is not split
 * over workgroups).  Equal weights and equicorrelation only (caller weights and a general correlation matrix:
 * smc_basket_price_general, below; path-dependent basket payoffs: smc_basket_price_paths, below). */
#define SMC_BASKET_PRICE_COLS 18
int32_t smc_basket_price(const double* contracts_dev /*[B][3A+4]*/, int64_t n_contracts, int32_t n_assets,
                         int32_t timesteps, int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                         int64_t ordinal0, int32_t math, int32_t normalization,
                         double* prices_dev /*[B][18]*/, double* terminal_sum_dev /*[B][A] or NULL*/, void* stream);
/* "basket_price_kernel(raw)", "basket_price_kernel(lds)", "basket_price_kernel(replay)" or "unsupported" (a
 * call smc_basket_price rejects).  Static string, no device call. */
const char* smc_basket_price_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                    int32_t normalization);

/* ---- batched Greeks (ABI 19) ----------------------------------------------------
 * Pathwise sensitivities of the European put and call smc_gbm_price averages, for B contracts in ONE launch:
 * the price call's workgroup per contract, streams (contract b uses ordinal (*ordinal_dev or 0) + ordinal0 + b),
 * geometry, modes and fixed sum order, so the block is bit-identical run to run, under any split of the batch
 * and in every mode.  SMC_SCHEME_LOG_EULER only: its terminal value x alone gives the path's log return
 * L = log(x / X0) = mu T + v sqrt(dt) sum z and with it every derivative below; SMC_SCHEME_SIMPLE_EULER is
 * rejected (SMC_ERR_INVALID_ARGUMENT), because its reflected step |x (1 + a + b z)| is not a function of the
 * terminal value.  The estimators are the derivatives of the estimator smc_gbm_price computes, including,
 * under SMC_NORM_NORMALIZE, the dependence of the scale F / mean(x) on the parameter.
 * Per contract, each constant in f64 from the row X0 K T r d v, then rounded to the sim dtype Real:
 *   F, df, K     as the price call's (F = X0 exp((r - d) T), df = exp(-r T), evaluated in Real)
 *   s            F / Real(sumx / P) under NORMALIZE, 1 under RAW      mu = r - d - v^2 / 2
 *   ix0 = Real(1 / X0)    cv = Real(1 / v), 0 if v == 0    cT = Real(1 / (2 T)), 0 if T == 0
 *   crho = df * (Real(T) * K)    rr = Real(r)
 *   RAW:        av = Real(-mu T / v - v T), 0 if v == 0         aT = Real(mu / 2)
 *   NORMALIZE:  Lbar = sumxl / sumx (f64)   av = Real(-Lbar / v), 0 if v == 0
 *               aT = Real(-Lbar / (2 T) + (r - d)), Real(r - d) if T == 0
 *   sumx  = the f64 sum of the raw terminal values (the price call's column 7, bit for bit)
 *   sumxl = sum over the paths of f64(x * L) (NORMALIZE only), L = log(x / Real(X0)) in Real: the portable f32
 *           log, v_log_f32 times ln 2 under SMC_MATH_HW, the library log in f64.
 * Per path, all in Real, every operation rounded (no fused multiply-add), each value cast to f64 and
 * averaged over the P paths:
 *   xs = x * s     ip = K - xs > 0     ic = xs - K > 0
 *   put = df * max(K - xs, 0)    call = df * max(xs - K, 0)    w = df * xs
 *   hv = L * cv + av  (d ln xs / d v)       hT = L * cT + aT  (d ln xs / d T)
 *   delta  put: ip ? -(w * ix0) : 0         call: ic ? w * ix0 : 0
 *   vega   put: ip ? -(w * hv) : 0          call: ic ? w * hv : 0
 *   rho    put: ip ? -crho : 0              call: ic ? crho : 0
 *   theta  put: rr * put + (ip ? w * hT : 0)   call: rr * call - (ic ? w * hT : 0)    (= -dV/dT, per year)
 * gamma is not an estimator of its own: gamma = vega / (v T X0^2) in f64 (the lognormal identity, exact for the
 * log-Euler terminal law), its standard error likewise; both 0 when v T == 0.
 * greeks_dev [B][26]:
 *    0 /  1 delta put / call       2 /  3 vega put / call       4 /  5 rho put / call
 *    6 /  7 theta put / call       8 /  9 gamma put / call
 *   10..19 the standard errors of columns 0..9 (the price call's formula; 0 at P = 1)
 *   20 / 21 put / call price, 22 / 23 their standard errors: the price call's columns 0, 1, 3, 4 bit for bit
 *   24 sumx: the price call's column 7 bit for bit         25 sumxl (0 under RAW).
 * Conventions: v == 0 gives vega = gamma = 0 (and errors 0); T == 0 drops theta's hT * (1 / (2 T)) term and gives
 * gamma = 0; P == 1 gives every standard error 0.  The standard errors take the P terms as independent: under
 * NORMALIZE they leave out the sampling error of the shared s and Lbar.  NORMALIZE needs the terminal values twice: parked in LDS
 * while the price call would park them (up to 144 KiB), else simulated a second time; SMC_PRICE_REPLAY forces
 * the latter.  scheme takes SMC_MATH_HW (f32 only) and SMC_PRICE_REPLAY; SMC_MATH_REF and any other bit are
 * rejected.  Checks, in this order and all before the empty batch (n_contracts = 0: SMC_OK, nothing touched)
 * is accepted: the price call's (NULL contracts_dev, shape, dtype; NULL greeks_dev; bad scheme or unknown
 * flag; SMC_MATH_REF; SMC_MATH_HW with f64; bad normalization), then the simple-Euler rejection.
 * Stream-ordered: no allocation, no synchronisation, capturable into a graph.  Contract values are not
 * validated on the device, as elsewhere: X0 <= 0 gives NaN.  B below the CU count leaves CUs idle.
 * Out of scope: simple Euler; Greeks of the path-dependent payoffs (the equal-weight basket's are
 * smc_basket_greeks, below); likelihood-ratio or second-order pathwise gamma; cross-Greeks. */
#define SMC_GREEKS_COLS 26
int32_t smc_gbm_greeks(const double* contracts_dev, int64_t n_contracts, int32_t timesteps, int64_t n_paths,
                       uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t scheme,
                       int32_t normalization, int32_t dtype, double* greeks_dev /*[B][26]*/, void* stream);
/* "greeks_kernel(raw)", "greeks_kernel(lds)", "greeks_kernel(replay)" or "unsupported" (a call smc_gbm_greeks
 * rejects, simple Euler among them).  Static string, no device call. */
const char* smc_gbm_greeks_kernel(int32_t timesteps, int64_t n_paths, int32_t scheme, int32_t normalization,
                                  int32_t dtype);

/* ---- batched basket Greeks (ABI 20) ---------------------------------------------
 * Pathwise sensitivities of the equal-weight basket put and call smc_basket_price averages, for B contracts of
 * A assets in ONE launch: the price call's workgroup per contract (512 lanes), contract rows ([B][3A+4]: K, T, r,
 * rho, X0[A], d[A], v[A]), streams (contract b uses ordinal (*ordinal_dev or 0) + ordinal0 + b), Cholesky factor,
 * packed f32 step, chunk and validity handling (any n_paths >= 1) and fixed sum orders, so the block is bit-identical
 * run to run, under any split of the batch, with the ordinal on the host or on the device, and in the lds and replay
 * modes.  The A terminal values x_i of a path give its log returns L_i = log(x_i / X0_i) = mu_i T + v_i W_i and
 * with them every derivative below; the estimators are the derivatives of the estimator smc_basket_price
 * computes, including, under SMC_NORM_NORMALIZE, the dependence of the scales F_i / mean(x_i) on the parameter.
 * Per contract, each constant in f64 from the row (every f64 operation rounded, in the order written), then
 * rounded to f32:
 *   K, df, F_i, s_i, wA   exactly smc_basket_price's (s_i = F_i / f32(tot_i / P) under NORMALIZE, 1 under RAW)
 *   mu_i = r - d_i - 0.5 v_i v_i    ix0_i = f32(1 / X0_i)    cv_i = f32(1 / v_i), 0 if v_i == 0
 *   cT = f32(1 / (2 T)), 0 if T == 0    crho = df * (f32(T) * K)    rr = f32(r)
 *   Lc   the engine's Banachiewicz factor of (1 - rho) I + rho 11^T (f64)
 *   dL   its derivative in rho, statement by statement: for i, for k <= i: ds = (i == k ? 0 : 1), then for m < k:
 *        ds = ds - (dL_im Lc_km + Lc_im dL_km);  dL_ii = ds / (2 Lc_ii),  dL_ik = (ds - Lc_ik dL_kk) / Lc_kk
 *   G    = dL Lc^-1 (lower triangular), row i from k = i down to 0: g = dL_ik, then for m = k + 1 .. i:
 *        g = g - G_im Lc_mk;  G_ik = g / Lc_kk.  dW / drho = G W for the correlated Brownian sums W = Lc (driver sums).
 *   g_ik = f32(v_i G_ik / v_k) for k <= i
 *   g0_i = f32(-(v_i gs_i)), gs_i = sum_{k <= i} G_ik mu_k T / v_k (from 0, in k order)
 *        (any v_k == 0: every g_ik and g0_i is 0, see the conventions)
 *   RAW:        av_i = f32(-mu_i T / v_i - v_i T), 0 if v_i == 0    aT_i = f32(mu_i / 2)    ac_i = 0
 *   NORMALIZE:  Lbar_i = sxl_i / tot_i (f64)    av_i = f32(-Lbar_i / v_i), 0 if v_i == 0
 *               aT_i = f32(-Lbar_i / (2 T) + (r - d_i)), f32(r - d_i) if T == 0    ac_i = f32(-sxc_i / tot_i)
 * Per path, all in f32, every operation rounded (no fused multiply-add):
 *   L_i = log(x_i / f32(X0_i))  (the portable f32 log; v_log_f32 times ln 2 under SMC_MATH_HW)
 *   c_i = (..((g0_i + g_i0 L_0) + g_i1 L_1) ..) + g_ii L_i     (v_i times d W_i / d rho)
 *   xs_i = x_i s_i    bk = (((0 + xs_0) + xs_1) + ...) wA    ip = K - bk > 0    ic = bk - K > 0
 *   put = df max(K - bk, 0)    call = df max(bk - K, 0)    w_i = (df * xs_i) * wA
 *   hv_i = L_i * cv_i + av_i    hT_i = L_i * cT + aT_i    hc_i = c_i + ac_i
 *   sT = ((0 + w_0 * hT_0) + w_1 * hT_1) + ...    sC = ((0 + w_0 * hc_0) + w_1 * hc_1) + ...
 *   delta_i      put: ip ? -(w_i * ix0_i) : 0     call: ic ? w_i * ix0_i : 0       (d / d X0_i)
 *   vega_i       put: ip ? -(w_i * hv_i) : 0      call: ic ? w_i * hv_i : 0        (d / d v_i)
 *   rho          put: ip ? -crho : 0              call: ic ? crho : 0              (d / d r)
 *   theta        put: rr * put + (ip ? sT : 0)    call: rr * call - (ic ? sT : 0)  (-d / d T, per year)
 *   correlation  put: ip ? -sC : 0                call: ic ? sC : 0                (d / d rho of the equicorrelation)
 * each cast to f64 and added with its square (f64); a column's sum runs per lane over its chunks and paths in
 * order, then the wave butterfly, then waves 0..7.
 * greeks_dev [B][2n + 4], n = 4A + 6:
 *   0 .. A-1 / A .. 2A-1 delta put / call      2A .. 3A-1 / 3A .. 4A-1 vega put / call
 *   4A, 4A+1 rho put / call    4A+2, 4A+3 theta put / call    4A+4, 4A+5 correlation put / call
 *   n .. 2n-1 the standard errors of columns 0 .. n-1 (the price call's formula; 0 at P = 1)
 *   2n, 2n+1 put / call price: smc_basket_price's columns 0 and 1 bit for bit
 *   2n+2, 2n+3 their standard errors: smc_basket_price's columns 6 and 7 bit for bit.
 * sums_dev (may be NULL) [B][3][A] f64: tot_i (smc_basket_price's terminal_sum_dev bit for bit), then
 * sxl_i = sum_p f64(x_i * L_i) and sxc_i = sum_p f64(x_i * c_i) (NORMALIZE; both 0 under RAW; the columns' sum order).
 * Conventions: v_i == 0 gives vega_i = 0 and its error 0.  Any v_i == 0 with A > 1: the drivers cannot be recovered
 * from a deterministic asset, so the four correlation columns (values and errors) are written as NaN, computed
 * with g = g0 = 0 (sxc = 0).  A == 1: there is no correlation, G = 0 and the correlation columns are exactly 0
 * (also at v == 0).  T == 0 drops the cT term.  P == 1 gives every standard error 0.  The standard errors take the P
 * terms as independent (they leave out the sampling error of the shared s_i, Lbar_i and ac_i).  Contract values are
 * not validated otherwise: at a singular matrix (rho = 1) the correlation columns and sxc may be non-finite, the
 * rest stays finite for A <= 2.
 * Modes: RAW takes the sums as the paths finish.  NORMALIZE needs the terminal values again once tot, sxl and sxc are
 * known: parked in LDS (x only; L and c are recomputed from the same bits) while A * roundup4(P) * 4 bytes and 6848
 * bytes of scratch fit in 144 KiB, else simulated again; SMC_PRICE_REPLAY forces the latter.  For A <= 4 all 4A + 8
 * sums are taken in one payoff pass; for A = 5..8 the registers do not hold them beside the path loop, so the columns
 * are taken 8 per-path terms at a time (terms in column order, the prices last) in ceil((4A + 8) / 8) payoff passes,
 * after a pass for tot alone and (NORMALIZE) one for sxl and sxc, each over the parked values, or over paths simulated
 * again (replay, and RAW too): the same values and each column's one order in every mode.
 * math: 0 (portable, CPU-reproducible) or SMC_MATH_HW, optionally | SMC_PRICE_REPLAY; any other bit is rejected.
 * Checks, in smc_basket_price's order and all before the empty batch (n_contracts = 0: SMC_OK, nothing touched) is
 * accepted.  SMC_ERR_INVALID_ARGUMENT: NULL contracts_dev, NULL greeks_dev, n_assets outside 1..8, bad math, bad
 * normalization.  SMC_ERR_INVALID_SHAPE: n_contracts < 0 or >= 2^31, timesteps <= 0, n_paths <= 0 or >= 2^40.
 * Stream-ordered: no allocation, no synchronisation, capturable into a graph.  B below the CU count leaves CUs idle.
 * Out of scope: Greeks of the best-of / worst-of payoffs; gammas and cross-gammas (no diagonal lognormal identity
 * holds for a basket); a float64 basket engine; likelihood-ratio estimators.  The Greeks of the weighted,
 * general-correlation basket and the sensitivities to single correlation entries are smc_basket_greeks_general, below. */
int32_t smc_basket_greeks(const double* contracts_dev /*[B][3A+4]*/, int64_t n_contracts, int32_t n_assets,
                          int32_t timesteps, int64_t n_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                          int64_t ordinal0, int32_t math, int32_t normalization,
                          double* greeks_dev /*[B][8A+16]*/, double* sums_dev /*[B][3A] or NULL*/, void* stream);
/* "basket_greeks_kernel(raw)", "basket_greeks_kernel(lds)", "basket_greeks_kernel(replay)" or "unsupported" (a
 * call smc_basket_greeks rejects).  Static string, no device call. */
const char* smc_basket_greeks_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                     int32_t normalization);
/* Doubles per contract of greeks_dev: 8 n_assets + 16; -1 for n_assets outside 1..8. */
int32_t smc_basket_greeks_cols(int32_t n_assets);

/* ---- weighted, general-correlation basket pricing (ABI 21) ----------------------
 * smc_basket_price with the two things a real index or spread has of its own: weights and a full correlation
 * matrix, per contract or shared.  Taken unchanged from smc_basket_price: the contract rows ([B][3A+4]: K, T, r,
 * rho, X0[A], d[A], v[A]), the streams (contract b uses ordinal (*ordinal_dev or 0) + ordinal0 + b), the 512-lane
 * workgroup per contract, the chunking and the handling of any n_paths >= 1, the raw / lds / replay modes, the
 * fixed sum orders, the 18 columns of prices_dev (SMC_BASKET_PRICE_COLS), terminal_sum_dev and math (0 or
 * SMC_MATH_HW, optionally | SMC_PRICE_REPLAY).  New, for contract b:
 *   weights      w_i = f32(weights_dev[b * weights_stride + i]); f32(1.0 / A) when weights_dev is NULL.  Stride 0
 *                shares row 0 with every contract.  Any finite value is taken, negatives included (spread and
 *                exchange options); the weights are not normalised.
 *   correlation  for k < i, C_ik = corr_dev[b * corr_stride + i (i - 1) / 2 + k]: the strict lower triangle row by
 *                row, (1,0), (2,0), (2,1), (3,0), ...  When corr_dev is NULL, C_ik is the row's rho; otherwise the
 *                rho column is ignored.  C_ii = 1.  Stride 0 shares row 0.  At A = 1 nothing is read.
 *   factor       the engine's Banachiewicz statements with rho replaced by C_ik, in f64, by one thread, in LDS:
 *                for i, for k <= i: s = (i == k ? 1 : C_ik); for m < k: s = s - L_im L_km;
 *                L_ik = i == k ? sqrt(s > 0 ? s : 0) : s / L_kk.  Step coefficients as smc_basket_price's.
 * Per path, in f32, every operation rounded (no fused multiply-add), with s_i, tot_i, F_i, df and K exactly
 * smc_basket_price's:
 *   xs_i = x_i s_i    t_i = w_i xs_i    bk = ((0 + t_0) + t_1) + ...    mx = max_i xs_i    mn = min_i xs_i
 * (mx and mn are over the unweighted xs_i).  Payoffs, sums, standard errors and the exercise share are as in
 * smc_basket_price; columns 16 / 17 use Fb = ((0 + w_0 F_0) + w_1 F_1) + ...
 * What follows bit for bit: corr_dev with every entry equal to rho is corr_dev = NULL; with that correlation and
 * equal weights (NULL or explicit 1 / A) terminal_sum_dev and the rainbow columns 2..5, 8..11, 13, 14 are
 * smc_basket_price's for every A, and the whole block is for A in {1, 2, 4, 8}, where f32(1 / A) is a power of two
 * (sum (w xs_i) = (sum xs_i) w exactly); stride 0 is the same row materialised B times; lds is replay; run to
 * run, any split of the batch, the ordinal on the host or on the device.
 * NORMALIZE parks the terminal values in LDS while A * roundup4(P) * 4 bytes and this kernel's 2112 bytes of
 * scratch (smc_basket_price's: the factor is built from global memory, the weights stay in registers) fit in
 * 144 KiB, else simulates a second time; SMC_PRICE_REPLAY forces the latter.
 * Checks: smc_basket_price's, in its order; then SMC_ERR_INVALID_ARGUMENT for a non-NULL weights_dev whose
 * weights_stride is neither 0 nor >= A, then for a non-NULL corr_dev whose corr_stride is neither 0 nor
 * >= A (A - 1) / 2; all before the empty batch (n_contracts = 0: SMC_OK, nothing touched) is accepted.
 * Stream-ordered: no allocation, no synchronisation, capturable into a graph.  Nothing is validated on the
 * device, as elsewhere: a matrix that is not positive definite (the factor takes sqrt(max(s, 0)) and divides by
 * it) or a non-finite weight gives non-finite or meaningless rows; check on the host if the input is not trusted.
 * Out of scope: weights or a general correlation in the training targets; a float64 basket engine.  Greeks and correlation
 * sensitivities: smc_basket_greeks_general, below; Asian, barrier and lookback payoffs: smc_basket_price_paths, below. */
int32_t smc_basket_price_general(const double* contracts_dev /*[B][3A+4]*/,
                                 const double* weights_dev /*rows of A, or NULL*/, int64_t weights_stride,
                                 const double* corr_dev /*rows of A(A-1)/2, or NULL*/, int64_t corr_stride,
                                 int64_t n_contracts, int32_t n_assets, int32_t timesteps, int64_t n_paths,
                                 uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                                 int32_t normalization, double* prices_dev /*[B][18]*/,
                                 double* terminal_sum_dev /*[B][A] or NULL*/, void* stream);
/* "basket_general_kernel(raw)", "basket_general_kernel(lds)", "basket_general_kernel(replay)" or "unsupported"
 * (a call smc_basket_price_general rejects).  Static string, no device call. */
const char* smc_basket_price_general_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                            int32_t normalization);

/* ---- Greeks of the weighted, general-correlation basket (additive under ABI 21) ----
 * smc_basket_greeks for the basket smc_basket_price_general prices: it relates to smc_basket_greeks exactly as
 * smc_basket_price_general relates to smc_basket_price.  Inputs: weights_dev, weights_stride, corr_dev, corr_stride
 * with smc_basket_price_general's meaning (w_i = f32 of the caller's f64, f32(1.0 / A) when NULL; the packed strict
 * lower triangle (1,0), (2,0), (2,1), (3,0), ...; C_ik = the row's rho when NULL; stride 0 shares row 0; nothing read
 * at A = 1) and its factor L (the Banachiewicz statements on C_ik); everything else is smc_basket_greeks's.
 * With np = A (A - 1) / 2 pairs, n = 4A + 4 + 2 np, greeks_dev is [B][2n + 4] (2 A^2 + 6 A + 12 doubles):
 *   0 .. A-1 / A .. 2A-1 delta put / call      2A .. 3A-1 / 3A .. 4A-1 vega put / call
 *   4A, 4A+1 rho put / call    4A+2, 4A+3 theta put / call
 *   4A+4 .. 4A+3+np     d put / d C_jk, pair q = j (j - 1) / 2 + k in the packed order (1,0), (2,0), (2,1), (3,0), ...
 *   4A+4+np .. n-1      d call / d C_jk in the same order
 *   n .. 2n-1 the standard errors of columns 0 .. n-1 (the price call's formula; 0 at P = 1)
 *   2n, 2n+1 put / call price: smc_basket_price_general's columns 0 and 1 bit for bit
 *   2n+2, 2n+3 their standard errors: smc_basket_price_general's columns 6 and 7 bit for bit.
 * d / d C_jk is the derivative with respect to the pair: C_jk and C_kj move together and the matrix stays symmetric
 * (it is the derivative in the one packed entry the factor reads).  smc_basket_greeks's correlation column moves all
 * pairs together in this way, so where every entry equals rho the pair columns sum to it (to rounding).
 * The drivers do not depend on C: with W = L (driver sums), dW / dC_jk = G^jk W, G^jk = (dL / dC_jk) L^-1 lower
 * triangular with rows i < j zero, and c_i^jk = d ln x_i / d C_jk follows from the A terminal logs alone.
 * Per contract, each constant in f64 (every f64 operation rounded, in the order written), then rounded to f32; thread q
 * of the workgroup takes pair q:
 *   K, df, F_i, s_i, w_i   exactly smc_basket_price_general's
 *   mu_i, ix0_i, cv_i, cT, crho, rr, av_i, aT_i   exactly smc_basket_greeks's, Lbar_i = M_ii / tot_i under NORMALIZE
 *   dL^jk  the derivative of the factor's statements with the seed 1 at (j, k): for i, for m <= i:
 *          ds = (i == j && m == k ? 1 : 0), then for u < m: ds = ds - (dL_iu L_mu + L_iu dL_mu);
 *          dL_ii = ds / (2 L_ii),  dL_im = (ds - L_im dL_mm) / L_mm
 *   G^jk   = dL^jk L^-1, row i from m = i down to 0: g = dL_im, then for u = m + 1 .. i: g = g - G_iu L_um;
 *          G_im = g / L_mm  (smc_basket_greeks's two recursions with another seed)
 *   g_im^jk = f32(v_i G_im^jk / v_m) for m <= i
 *   g0_i^jk = f32(-(v_i gs_i)), gs_i = sum_{m <= i} G_im^jk mu_m T / v_m (from 0, in m order)
 *          (any v_m == 0: every g and g0 is 0, see the conventions)
 *   RAW:        ac_i^jk = 0
 *   NORMALIZE:  M_im = sum_p f64(x_i * L_m) for m <= i (the columns' sum order; M_ii is smc_basket_greeks's sxl_i), and
 *               ac_i^jk = f32(-((..((f64(g0_i^jk) + f64(g_i0^jk) * (M_i0 / tot_i)) + f64(g_i1^jk) * (M_i1 / tot_i)) ..)
 *                              + f64(g_ii^jk) * (M_ii / tot_i)))
 *               from the f32 g and g0 the paths use: minus the x_i-weighted mean of c_i^jk over the paths, because c^jk
 *               is linear in the logs.
 * Per path, all in f32, every operation rounded (no fused multiply-add):
 *   L_i = log(x_i / f32(X0_i))  (the portable f32 log; v_log_f32 times ln 2 under SMC_MATH_HW)
 *   xs_i = x_i s_i    bk = ((0 + w_0 * xs_0) + w_1 * xs_1) + ...    ip = K - bk > 0    ic = bk - K > 0
 *   put = df max(K - bk, 0)    call = df max(bk - K, 0)    wt_i = (df * xs_i) * w_i
 *   hv_i = L_i * cv_i + av_i    hT_i = L_i * cT + aT_i    sT = ((0 + wt_0 * hT_0) + wt_1 * hT_1) + ...
 *   c_i^jk = (..((g0_i^jk + g_i0^jk * L_0) + g_i1^jk * L_1) ..) + g_ii^jk * L_i     for i >= j
 *   sC^jk = ((0 + wt_j * (c_j^jk + ac_j^jk)) + wt_{j+1} * (c_{j+1}^jk + ac_{j+1}^jk)) + ...   up to i = A - 1
 *   delta_i      put: ip ? -(wt_i * ix0_i) : 0    call: ic ? wt_i * ix0_i : 0
 *   vega_i       put: ip ? -(wt_i * hv_i) : 0     call: ic ? wt_i * hv_i : 0
 *   rho          put: ip ? -crho : 0              call: ic ? crho : 0
 *   theta        put: rr * put + (ip ? sT : 0)    call: rr * call - (ic ? sT : 0)
 *   pair (j, k)  put: ip ? -sC^jk : 0             call: ic ? sC^jk : 0
 * each cast to f64 and added with its square (f64); a column's sum runs per lane over its chunks and paths in order,
 * then the wave butterfly, then waves 0..7.  A negative weight flips the signs by itself; nothing takes |w|.
 * sums_dev (may be NULL) [B][A + A (A + 1) / 2] f64: tot_i (smc_basket_price_general's terminal_sum_dev bit for bit),
 * then M_im at A + i (i + 1) / 2 + m (M_00, M_10, M_11, M_20, ...; all 0 under RAW).
 * What follows bit for bit: the price columns and tot as above; lds is replay; run to run, any split of the batch, the
 * ordinal on the host or on the device; stride 0 is the row materialised B times; corr_dev with every entry equal to
 * rho is corr_dev = NULL; and with that correlation and equal weights (NULL or explicit 1 / A) the delta, vega, rho and
 * theta columns with their errors are smc_basket_greeks's for A in {1, 2, 4, 8}, where f32(1 / A) is a power of two.
 * Conventions (smc_basket_greeks's): v_i == 0 gives vega_i = 0 and its error 0.  Any v_i == 0 with A > 1 writes every
 * pair column, values and errors, as NaN (computed with g = g0 = 0).  A == 1 has no pair column.  T == 0 drops the cT
 * term.  P == 1 gives every standard error 0.  Nothing is validated on the device: a matrix that is not positive
 * definite or a non-finite weight gives non-finite or meaningless rows.
 * Modes and passes: the n + 2 per-path terms are taken in kernel order (the 4A + 4 delta, vega, rho and theta terms as
 * columns, then put and call of pair 0, of pair 1, ..., then the two prices) in payoff passes of all of them for
 * A <= 3, 12 for A = 4 and 8 for A = 5..8, i.e. 1, 1, 1, 3, 6, 8, 10, 12 passes for A = 1..8.  Before them, NORMALIZE
 * takes one pass for tot and M together (A <= 4) or one for tot and one for M (A >= 5); RAW takes tot with its single
 * payoff pass (A <= 3) or in a pass of its own (A >= 4).  The first pass simulates; every later one reads the terminal
 * values parked in LDS (x only), or simulates again (replay, and RAW too): the same values and each column's one order
 * in every mode.  The parked block is used while A * roundup4(P) * 4 bytes and this kernel's 15968 bytes of scratch
 * (pass partials, the factor, the pass-1 partials and totals, 64 f32 per-asset and 28 x 80 f32 per-pair constants) fit
 * in 144 KiB; SMC_PRICE_REPLAY forces replay.
 * math: 0 or SMC_MATH_HW, optionally | SMC_PRICE_REPLAY; any other bit is rejected.
 * Checks, all before the empty batch (n_contracts = 0: SMC_OK, nothing touched) is accepted: smc_basket_greeks's in
 * its order (NULL contracts_dev, NULL greeks_dev, n_assets, math, normalization: SMC_ERR_INVALID_ARGUMENT; n_contracts,
 * timesteps, n_paths: SMC_ERR_INVALID_SHAPE), then smc_basket_price_general's two stride checks
 * (SMC_ERR_INVALID_ARGUMENT), weights first.
 * Stream-ordered: no allocation, no synchronisation, capturable into a graph.
 * Out of scope: Greeks of the best-of / worst-of payoffs; gammas and cross-gammas; sensitivities to the weights; a
 * switch that skips the pair columns; weights or a general correlation in the training targets; a float64 basket
 * engine; likelihood-ratio estimators. */
int32_t smc_basket_greeks_general(const double* contracts_dev /*[B][3A+4]*/,
                                  const double* weights_dev /*rows of A, or NULL*/, int64_t weights_stride,
                                  const double* corr_dev /*rows of A(A-1)/2, or NULL*/, int64_t corr_stride,
                                  int64_t n_contracts, int32_t n_assets, int32_t timesteps, int64_t n_paths,
                                  uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                                  int32_t normalization, double* greeks_dev /*[B][2A^2+6A+12]*/,
                                  double* sums_dev /*[B][A + A(A+1)/2] or NULL*/, void* stream);
/* "basket_greeks_general_kernel(raw)", "basket_greeks_general_kernel(lds)", "basket_greeks_general_kernel(replay)"
 * or "unsupported" (a call smc_basket_greeks_general rejects).  Static string, no device call. */
const char* smc_basket_greeks_general_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                             int32_t normalization);
/* Doubles per contract of greeks_dev: 2 A^2 + 6 A + 12; -1 for n_assets outside 1..8. */
int32_t smc_basket_greeks_general_cols(int32_t n_assets);

/* ---- path-dependent basket pricing (additive under ABI 21) -----------------------
 * Asian, barrier and lookback options on the basket level, and worst-of barrier structures, for B contracts in ONE
 * launch: smc_gbm_price_paths for the basket smc_basket_price_general prices.  The T monitoring dates are the T grid
 * points of the simulation (X0 is not monitored); no row of the [A][T][P] block is ever stored.
 * Taken unchanged from smc_basket_price_general: the contract rows ([B][3A+4]), the streams and the ordinal handling,
 * weights_dev / weights_stride (NULL = f32(1.0 / A), stride 0 shares row 0, any sign), corr_dev / corr_stride (the
 * packed strict lower triangle; NULL = the row's rho) and the factor, the step coefficients, the 512-lane workgroup
 * per contract, 4 paths per lane, 2048-path chunks, validity for any n_paths >= 1, A in 1..8, K and df.
 * Monitored values, for asset i and row t: xs_it = x_it s_it, rounded to f32.  s_it = 1 under SMC_NORM_RAW.  Under
 * SMC_NORM_NORMALIZE s_it = F_it / f32(rowsum_it / f64(P)) with F_it = f32(X0_i) exp(f32(r - d_i) f32(tau_t)),
 * tau_t = (t + 1) (T / timesteps) in f64 for t < timesteps - 1 and tau = T exactly for the last row, and rowsum_it in
 * the order smc_basket_price_general takes tot_i: the lane's valid values left to right in f32 from 0, cast to f64 and
 * added per lane over its chunks, the wave butterfly xor 32..1, waves 0..7.  So the last row's sum, scale and forward
 * are that call's tot_i, s_i and F_i bit for bit, and terminal_sum_dev ([B][A] or NULL) is its output bit for bit.
 * Per path, all in f32, every operation rounded (no fused multiply-add), rows t = 0 .. timesteps - 1 in order:
 *   b_t = ((0 + w_0 xs_0t) + w_1 xs_1t) + ...      m_t = min_i xs_it  (unweighted, as the price call's mn)
 *   avg = (((0 + b_0) + b_1) + ...) / f32(timesteps)      mxb = max_t b_t      mnb = min_t b_t
 *   ko = any_t (b_t <= lower || b_t >= upper)      wko = any_t (m_t <= worst_lower)
 * with (lower, upper, worst_lower) = f32 of barriers_dev[b][0..2]; barriers_dev NULL means (-inf, +inf, -inf).  The
 * comparisons are plain ones: a side is switched off with -inf or +inf, not with 0 (a spread's level may be
 * negative).  Payoffs are df max(. , 0), cast to f64 and added with their squares.  prices_dev [B][25]:
 *    0 / 1  Asian basket put K - avg / call avg - K
 *    2 / 3  knock-out basket put / call: 0 if ko, else K - b_last / b_last - K
 *    4 / 5  lookback basket put K - mnb / call mxb - K
 *    6 / 7  worst-of put / call knocked out on the worst asset: 0 if wko, else K - m_last / m_last - K
 *    8 / 9  European basket put / call (smc_basket_price_general's columns 0 / 1 bit for bit)
 *   10..19  the standard errors of columns 0..9 (the price call's formula; 0 at P = 1)
 *   20 mean of avg    21 share of paths with ko    22 share with wko    23 mean of mxb    24 mean of mnb
 * Knock-ins follow by difference: European minus knock-out for the basket columns, smc_basket_price_general's
 * worst-of columns 4 / 5 minus 6 / 7 for the worst-of ones.  Without barriers columns 2, 3, 12, 13 are 8, 9, 18, 19,
 * columns 6, 7, 16, 17 are the price call's 4, 5, 10, 11 and columns 21, 22 are 0, bit for bit; at timesteps = 1
 * columns 0, 1, 4, 5 and their errors are 8, 9 and theirs and 20, 23, 24 are the price call's column 12.
 * Each column's sum runs per lane over its chunks and paths in order, then the wave butterfly, then waves 0..7: the
 * block is bit-identical run to run, under any split of the batch, with the ordinal on the host or the device.
 * Passes.  RAW: one simulation.  NORMALIZE: the A * timesteps row sums are per-lane f64 accumulators in LDS
 * ([R][512]), R rows at a time in sweeps of floor(R / A) whole dates, each sweep simulating from row 0 to its last
 * row (a row's sum lies in one sweep, so sweep boundaries change no order); R is what fits in 144 KiB beside 2112
 * bytes of scratch and the A * timesteps f32 scales; a final simulation takes the payoffs.  For A = 5..8 the 25 sums
 * and the per-path state do not fit in registers beside the 4 A path values: the columns are then taken in three
 * groups over three payoff simulations ({Asian, European, 20}, {knock-out, worst-of knock-out, 21, 22}, {lookback,
 * 23, 24}); a sum belongs to one group and keeps its order.
 * math: 0 or SMC_MATH_HW.  SMC_PRICE_REPLAY is accepted and changes nothing (there is no parked mode: A T P values
 * do not fit in LDS); any other bit is rejected.
 * Checks: smc_basket_price_general's, in its order and with its status codes (NULL contracts_dev, NULL prices_dev,
 * n_assets, math, normalization: SMC_ERR_INVALID_ARGUMENT; n_contracts, timesteps, n_paths: SMC_ERR_INVALID_SHAPE;
 * weights_stride, corr_stride: SMC_ERR_INVALID_ARGUMENT); then SMC_ERR_INVALID_SHAPE for a NORMALIZE run whose
 * n_assets * timesteps scales do not fit the LDS table beside one date of accumulators; all before the empty batch
 * (n_contracts = 0: SMC_OK, nothing touched) is accepted.
 * Stream-ordered: no allocation, no synchronisation, no workspace, no atomics, capturable into a graph.  Nothing is
 * validated on the device (NaN barriers never knock; lower >= upper knocks every path).
 * Out of scope: continuous-monitoring corrections; geometric averages; per-asset barrier levels; a float64 basket engine; weights or a general correlation in the training targets. */
#define SMC_BASKET_PATH_COLS 25
int32_t smc_basket_price_paths(const double* contracts_dev /*[B][3A+4]*/,
                               const double* weights_dev /*rows of A, or NULL*/, int64_t weights_stride,
                               const double* corr_dev /*rows of A(A-1)/2, or NULL*/, int64_t corr_stride,
                               const double* barriers_dev /*[B][3] or NULL*/,
                               int64_t n_contracts, int32_t n_assets, int32_t timesteps, int64_t n_paths,
                               uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                               int32_t normalization, double* prices_dev /*[B][25]*/,
                               double* terminal_sum_dev /*[B][A] or NULL*/, void* stream);
/* "basket_path_kernel(raw)", "basket_path_kernel(replay)" or "unsupported" (a call smc_basket_price_paths
 * rejects).  Static string, no device call. */
const char* smc_basket_price_paths_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                          int32_t normalization);

/* ---- batched Greeks of the Asian and lookback options (additive under ABI 21) -----
 * Pathwise delta, vega, rho and theta of the Asian and fixed-strike lookback options smc_gbm_price_paths prices, with
 * standard errors, for B contracts in ONE launch.  The pathwise method is exact for these payoffs (they are Lipschitz
 * in the path); the knock-out payoffs are not (the knocked flag is discontinuous) and have no column here.  There is
 * no gamma: the lognormal identity vega = v T X0^2 gamma of smc_gbm_greeks holds for a function of the terminal value
 * only.  SMC_SCHEME_LOG_EULER only.
 * Taken unchanged from smc_gbm_price_paths: the contract rows, the streams and the ordinal handling, the 512-lane
 * workgroup per contract, 4 paths per lane, 2048-path chunks, validity for any n_paths >= 1, the monitoring dates
 * (the T grid points; X0 is not monitored), K, df, the row sums, F_t and the scales s_t.
 * Row t (0-based, steps = timesteps): x_t the raw value, xs_t = x_t s_t rounded to Real (s_t = 1 under RAW,
 * F_t / Real(sumx_t / P) under NORMALIZE), tau_t the f64 grid point of F_t (tau = (t + 1) (T / steps), the last one T
 * exactly), fr_t = (t + 1) / steps in f64, L_t = log(x_t / Real(X0)) (the portable f32 log; v_log_f32 times ln 2
 * under SMC_MATH_HW; the library log in f64), mu = r - d - v^2 / 2.
 * Per contract, each in f64 from the contract row, then rounded to Real: K, df (the price call's), ix0 = 1 / X0,
 * cv = 1 / v (0 if v == 0), cT = 1 / (2 T) (0 if T == 0), rr = r, Tr = T.
 * Per row, in f64, then rounded to Real (four tables in LDS: s_t and these three):
 *   tr_t = tau_t                                                        (d ln xs_t / d r)
 *   RAW:        av_t = -mu tau_t / v - v tau_t (0 if v == 0)            aT_t = mu / 2 * fr_t
 *   NORMALIZE:  Lbar_t = sumxl_t / sumx_t
 *               av_t = -Lbar_t / v (0 if v == 0)
 *               aT_t = -Lbar_t / (2 T) + (r - d) fr_t    ((r - d) fr_t if T == 0)
 * sumx_t is smc_gbm_price_paths' row sum bit for bit; sumxl_t = sum over the valid paths of f64(x_t * L_t) (the
 * product in Real, each product cast and added singly), per lane over its chunks, then the wave butterfly, then
 * waves 0..7.
 * Per path and row, every operation rounded in Real (no fused multiply-add):
 *   hv_t = L_t * cv + av_t          (d ln xs_t / d v)
 *   hT_t = L_t * cT + aT_t          (d ln xs_t / d T, all monitoring dates moving in proportion with T)
 *   sa += xs_t    sv += xs_t * hv_t    sT += xs_t * hT_t    sr += xs_t * tr_t
 *   if (xs_t > mx) { mx = xs_t; Lmx = L_t; tmx = t }      (strict: the first row wins a tie)
 *   if (xs_t < mn) { mn = xs_t; Lmn = L_t; tmn = t }
 * At the end of a path the underlying u and its derivatives gv, gT, gr:
 *   Asian          u = sa / steps    gv = sv / steps    gT = sT / steps    gr = sr / steps
 *   lookback call  u = mx    gv = mx * (Lmx * cv + av[tmx])    gT = mx * (Lmx * cT + aT[tmx])    gr = mx * tr[tmx]
 *   lookback put   the same with mn, Lmn, tmn
 * and, with ip = K - u > 0 and ic = u - K > 0:
 *   put = df * max(K - u, 0)        call = df * max(u - K, 0)
 *   delta  put: ip ? -((df * u) * ix0) : 0            call: ic ? (df * u) * ix0 : 0
 *   vega   put: ip ? -(df * gv) : 0                   call: ic ? df * gv : 0
 *   rho    put: -(Tr * put) - (ip ? df * gr : 0)      call: -(Tr * call) + (ic ? df * gr : 0)
 *   theta  put: rr * put + (ip ? df * gT : 0)         call: rr * call - (ic ? df * gT : 0)     (-d / d T, per year)
 * each cast to f64 and added with its square (f64); a column's sum runs per lane over its chunks and paths in
 * order, then the wave butterfly, then waves 0..7.  Under NORMALIZE these are the derivatives of the estimator
 * smc_gbm_price_paths computes: the dependence of every row scale F_t / mean(x_t) on the parameter is included
 * (that is Lbar_t); delta and rho need no correction, because x_t, F_t and the mean move alike.
 * greeks_dev [B][40]; inside every group of four the order is Asian put, Asian call, lookback put, lookback call:
 *    0..3  delta    4..7  vega    8..11  rho    12..15  theta
 *   16..31 the standard errors of columns 0..15 (the price call's formula; 0 at P = 1)
 *   32..35 the four prices: smc_gbm_price_paths' columns 0, 1, 4, 5 bit for bit (barriers_dev = NULL)
 *   36..39 their standard errors: its columns 8, 9, 12, 13 bit for bit.
 * The standard errors take the P terms as independent (they leave out the sampling error of the shared s_t and
 * Lbar_t).  Conventions: v == 0 gives cv = av_t = 0; T == 0 drops the cT term; P == 1 gives every standard error 0.
 * Passes.  RAW: the tables come from the contract row; one simulation (f32) takes all 40 sums.  NORMALIZE: pass 1
 * takes sumx_t and sumxl_t as per-lane f64 accumulators in LDS ([2 R][512] doubles) in sweeps of R rows, each sweep
 * simulating from row 0 to its last row; R is even, min(roundup2(T), what fits): the LDS a workgroup may take (144 KiB
 * in f32; 160 KiB less the 51,232-byte table image of the path math in f64) less 2560 bytes of scratch and the four
 * tables (4 roundup8(T sizeof(Real)) bytes), divided by 8192 and rounded down to even: 16 in f32 and 12 in f64 at
 * T = 16.  A sweep boundary changes no sum's order.  Then the payoff simulation re-creates the same streams.  In f64
 * the registers do not hold the 40 sums and the path state beside the step, so the Asian and the lookback columns are
 * taken in two payoff simulations; a sum belongs to one of them and keeps its order, so no value depends on that.
 * Checks, in smc_gbm_price_paths' order and all before the empty batch (n_contracts = 0: SMC_OK, nothing touched) is
 * accepted.  SMC_ERR_INVALID_ARGUMENT: NULL contracts_dev, bad dtype, NULL greeks_dev, a scheme with unknown bits,
 * SMC_MATH_REF, SMC_TRAIN_DYNAMIC or SMC_PRICE_REPLAY, SMC_MATH_HW with f64, bad normalization, then
 * SMC_SCHEME_SIMPLE_EULER.  SMC_ERR_INVALID_SHAPE: n_contracts < 0 or >= 2^31, timesteps <= 0, n_paths <= 0 or
 * >= 2^40; then, in both normalisations, timesteps whose four tables do not leave room for one sweep of two rows:
 * 2560 + 4 roundup8(T sizeof(Real)) + 16384 bytes above the LDS named above (T > 8032 in f32, T > 2927 in f64).
 * Stream-ordered: no allocation, no synchronisation, no workspace, no atomics, capturable into a graph.  B below the
 * CU count leaves CUs idle.
 * Out of scope: knock-out and knock-in Greeks (a pathwise estimator of them is biased); gamma and cross-Greeks;
 * simple Euler; SMC_MATH_REF; continuous-monitoring corrections. */
#define SMC_PATH_GREEKS_COLS 40
int32_t smc_gbm_greeks_paths(const double* contracts_dev, int64_t n_contracts, int32_t timesteps, int64_t n_paths,
                             uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t scheme,
                             int32_t normalization, int32_t dtype, double* greeks_dev /*[B][40]*/, void* stream);
/* "path_greeks_kernel(raw)", "path_greeks_kernel(replay)" or "unsupported" (a call smc_gbm_greeks_paths rejects).
 * Static string, no device call. */
const char* smc_gbm_greeks_paths_kernel(int32_t timesteps, int64_t n_paths, int32_t scheme, int32_t normalization,
                                        int32_t dtype);

/* ---- Greeks of the Asian and lookback basket options (additive under ABI 21) -----
 * Pathwise delta_i and vega_i per asset, rho and theta of the Asian and fixed-strike lookback options on the weighted
 * basket level that smc_basket_price_paths prices, with standard errors, for B contracts in ONE launch:
 * smc_gbm_greeks_paths' estimator, asset by asset.  An asset's volatility and spot move only that asset's rows
 * (x_it = X0_i exp(mu_i tau_t + v_i W_it), and W does not depend on them).  The knock-out and worst-of payoffs have no
 * column (a pathwise estimator of a knocked flag is biased); the European Greeks are smc_basket_greeks_general's.
 * Taken unchanged from smc_basket_price_paths, the same in every respect: the contract rows ([B][3A+4]), the streams
 * and the ordinal handling, weights_dev / weights_stride (NULL = f32(1.0 / A), stride 0 shares row 0, any sign),
 * corr_dev / corr_stride (the packed strict lower triangle; NULL = the row's rho) and cholesky_general's factor, the
 * step, one 512-lane workgroup per contract, 4 paths per lane, 2048-path chunks, validity for any n_paths >= 1, A in
 * 1..8, K, df, the row sums, F_it, s_it, xs_it, and the f32 order of b_t and avg.
 * Per contract, each in f64 from the contract row, then rounded to f32: K, df (the price call's), Tr = T, rr = r,
 * cT = 1 / (2 T) (0 if T == 0), steps = f32(timesteps); per asset ix0_i = 1 / X0_i, cv_i = 1 / v_i (0 if v_i == 0),
 * w_i, mu_i = r - d_i - v_i^2 / 2.
 * Row t (0-based): tau_t = (t + 1) (T / timesteps) in f64, the last one T exactly; fr_t = (t + 1) / timesteps in f64.
 * Per asset and row, in f64, then rounded to f32 (tables in LDS: s_it and av_it, aT_it per asset, tau_t per row):
 *   RAW:        s_it = 1    av_it = -mu_i tau_t / v_i - v_i tau_t (0 if v_i == 0)    aT_it = mu_i / 2 * fr_t
 *   NORMALIZE:  s_it = smc_basket_price_paths' scale bit for bit    Lbar_it = sumxl_it / sumx_it
 *               av_it = -Lbar_it / v_i (0 if v_i == 0)
 *               aT_it = -Lbar_it / (2 T) + (r - d_i) fr_t    ((r - d_i) fr_t if T == 0)
 * sumx_it is smc_basket_price_paths' row sum bit for bit; sumxl_it = sum over the valid paths of f64(x_it * L_it) (the
 * product in f32, each product cast and added singly), per lane over its chunks, then the wave butterfly, then waves
 * 0..7.
 * Per path and row, all in f32, every operation rounded (no fused multiply-add), assets i = 0 .. A - 1 in order:
 *   L_it = log(x_it / f32(X0_i))  (the portable f32 log; v_log_f32 times ln 2 under SMC_MATH_HW)
 *   xs_it = x_it * s_it (x_it under RAW)    wx_i = w_i * xs_it    b_t = ((0 + wx_0) + wx_1) + ...
 *   hv_i = L_it * cv_i + av_it      hT_i = L_it * cT + aT_it      rowT = ((0 + wx_0 * hT_0) + wx_1 * hT_1) + ...
 *   Asian:     sa += b_t    sd_i += wx_i    sv_i += wx_i * hv_i    sT += rowT    sr += b_t * tau_t
 *   lookback:  if (b_t > mx) { mx = b_t; tmx = t; keep x_it for every i }   (strict: the first row wins a tie)
 *              if (b_t < mn) { mn = b_t; tmn = t; keep x_it for every i }
 * At the end of a path, the underlying u and its derivatives:
 *   Asian     u = sa / steps    du_i = (sd_i / steps) * ix0_i    gv_i = sv_i / steps    gT = sT / steps
 *             gr = sr / steps   wd_i = df * du_i    wv_i = df * gv_i
 *   lookback  u = mx (call) or mn (put); with the kept x_i and the tables of row t* = tmx or tmn, wx_i, L_i, hv_i, hT_i
 *             as above:  wd_i = (df * wx_i) * ix0_i    wv_i = df * (wx_i * hv_i)
 *             gT = ((0 + wx_0 * hT_0) + wx_1 * hT_1) + ...    gr = u * tau_t*
 * and, with ip = K - u > 0, ic = u - K > 0, put = df * max(K - u, 0), call = df * max(u - K, 0):
 *   delta_i  put: ip ? -wd_i : 0                        call: ic ? wd_i : 0
 *   vega_i   put: ip ? -wv_i : 0                        call: ic ? wv_i : 0
 *   rho      put: -(Tr * put) - (ip ? df * gr : 0)      call: -(Tr * call) + (ic ? df * gr : 0)
 *   theta    put: rr * put + (ip ? df * gT : 0)         call: rr * call - (ic ? df * gT : 0)    (-d / d T, per year,
 *            all monitoring dates moving in proportion with T)
 * each cast to f64 and added with its square (f64); a column's sum runs per lane over its chunks and paths in order,
 * then the wave butterfly, then waves 0..7, sum k totalled by one thread.  A negative weight flips the signs by
 * itself; nothing takes |w|.
 * greeks_dev [B][16A+24].  Greek kinds g = 0 .. G - 1, G = 2A + 2: delta_0 .. delta_{A-1}, vega_0 .. vega_{A-1}, rho,
 * theta.  Payoffs q = 0 .. 3: Asian put, Asian call, lookback put (K - min_t b_t), lookback call (max_t b_t - K).
 *   4 g + q        Greek g of payoff q          4 G + 4 g + q   its standard error
 *   8 G + q        the price of payoff q: smc_basket_price_paths' columns 0, 1, 4, 5 bit for bit (barriers_dev NULL)
 *   8 G + 4 + q    its standard error: that call's columns 10, 11, 14, 15 bit for bit
 * At A = 1 this is smc_gbm_greeks_paths' 40-column layout.  The standard errors take the P terms as independent.
 * Conventions (smc_gbm_greeks_paths' and smc_basket_greeks_general's): v_i == 0 gives vega_i and its error 0; T == 0
 * drops the cT term; P == 1 gives every standard error 0; nothing is validated on the device.
 * Passes.  A payoff simulation takes at most 22 of the 8A + 12 terms.  A <= 4: two simulations, {Asian: every delta_i
 * and vega_i, rho, theta, price} and {lookback put and call, all of theirs}.  A = 5..8: passes of at most 16 terms,
 * {Asian: rho, theta, price}, then {Asian: delta_i, vega_i} over the assets in ranges of 4 (A = 5, 6: 0..3, 4..A-1) or
 * of 2 (A = 7, 8: 0..1, 2..3, 4..5, 6..A-1), {lookback put: every delta_i, rho, theta, price}, {lookback put: every
 * vega_i} and the same two for the lookback call: 7 simulations for A = 5, 6 and 9 for A = 7, 8.  A sum belongs to
 * one pass and keeps its one order, so no value depends on the plan.  NORMALIZE first takes the 2 A timesteps row sums (sumx, sumxl) as per-lane
 * f64 accumulators in LDS, in sweeps of whole dates (2A rows of 512 doubles per date), each sweep simulating from row
 * 0 to its last row; the dates per sweep are what fits in 144 KiB beside 3328 bytes of scratch and the tables
 * (roundup8(4 (3A + 1) timesteps) bytes).  There is no parked mode.
 * math: 0 or SMC_MATH_HW.  SMC_PRICE_REPLAY is accepted and changes nothing; any other bit is rejected.
 * Checks: smc_basket_price_paths' in its order and with its status codes, without the barrier argument (NULL
 * contracts_dev, NULL greeks_dev, n_assets, math, normalization: SMC_ERR_INVALID_ARGUMENT; n_contracts, timesteps,
 * n_paths: SMC_ERR_INVALID_SHAPE; weights_stride, corr_stride: SMC_ERR_INVALID_ARGUMENT); then, in both
 * normalisations, SMC_ERR_INVALID_SHAPE for a shape whose tables leave no room for one date of accumulators
 * (3328 + roundup8(4 (3A + 1) timesteps) + 8192 A bytes above 144 KiB); all before the empty batch (n_contracts = 0:
 * SMC_OK, nothing touched) is accepted.
 * Stream-ordered: no allocation, no synchronisation, no workspace, no atomics, no exchange between workgroups,
 * capturable into a graph.
 * Out of scope: correlation-pair sensitivities of these payoffs (the NORMALIZE correction would need A (A + 1) / 2
 * moment sums per row); knock-out and worst-of Greeks; gammas; sensitivities to the weights; terminal_sum_dev; a
 * float64 basket engine; continuous-monitoring corrections. */
int32_t smc_basket_greeks_paths(const double* contracts_dev /*[B][3A+4]*/,
                                const double* weights_dev /*rows of A, or NULL*/, int64_t weights_stride,
                                const double* corr_dev /*rows of A(A-1)/2, or NULL*/, int64_t corr_stride,
                                int64_t n_contracts, int32_t n_assets, int32_t timesteps, int64_t n_paths,
                                uint64_t mc_seed, const int64_t* ordinal_dev, int64_t ordinal0, int32_t math,
                                int32_t normalization, double* greeks_dev /*[B][16A+24]*/, void* stream);
/* "basket_path_greeks_kernel(raw)", "basket_path_greeks_kernel(replay)" or "unsupported" (a call
 * smc_basket_greeks_paths rejects).  Static string, no device call. */
const char* smc_basket_greeks_paths_kernel(int32_t n_assets, int32_t timesteps, int64_t n_paths, int32_t math,
                                           int32_t normalization);
/* Doubles per contract of greeks_dev: 16 A + 24; -1 for n_assets outside 1..8. */
int32_t smc_basket_greeks_paths_cols(int32_t n_assets);

/* ---- sliced batched pricing: one contract across workgroups (additive under ABI 21) -----
 * smc_gbm_price's 8 columns with each contract cut into W = ceil(n_paths / slice_paths) slices of slice_paths paths
 * (a positive multiple of 2048, the 512 x 4 chunk; the last slice is ragged and ends at n_paths), one 512-lane
 * workgroup per (contract, slice), B W workgroups in all: for one contract, or a few dozen, at a path count where
 * one workgroup per contract leaves most of the chip idle.
 * Taken unchanged from smc_gbm_price: the contract rows, the streams (contract b uses ordinal (*ordinal_dev or 0) +
 * ordinal0 + b; the lane group of paths p0..p0+3 the stream (seed, ordinal, p0 / 4, timesteps) with the contract-
 * global p0), the step, the payoff arithmetic in the sim dtype, SMC_MATH_HW (f32 only), the columns.
 * Order.  Inside a slice, smc_gbm_price's order over the slice's own chunks: per lane over the chunks with paths
 * ascending (the lane's 4 raw terminal values summed in the sim dtype first), the wave butterfly xor 32..1, waves
 * 0..7; lanes wholly past the slice end neither draw nor contribute.  A workgroup leaves six f64 partials in the
 * workspace: the raw terminal sum, put, call, underlying, put^2, call^2.  The six totals of a contract are slice 0's
 * value, then + slice 1, ..., + slice W - 1; the 8 columns are smc_gbm_price's closing arithmetic on the totals (the
 * standard errors, 0 at n_paths = 1; the intrinsic values; column 7 the total raw sum).  Under SMC_NORM_NORMALIZE
 * the scale is F / Real(total / n_paths) from the total raw sum.  So the block is bit-identical run to run, under any
 * split of the batch, and for slice_paths >= n_paths (W = 1) it is smc_gbm_price | SMC_PRICE_REPLAY's bit for bit; for
 * W > 1 the f64 sums are associated differently (by slice), the last bits of columns 0..4 and 7 may differ from
 * smc_gbm_price's, and in portable f32 math column 7 is the oracle's kernel-mode row sum at span = slice_paths.
 * Launches, in stream order on `stream`: SMC_NORM_RAW two (price_slice_kernel with the payoffs at scale 1, then
 * price_finish_kernel); SMC_NORM_NORMALIZE four (price_slice_kernel for the sums; price_finish_kernel for the totals;
 * price_slice_kernel again, replaying its slice's streams with the payoffs at the scale from the total;
 * price_finish_kernel for the columns).  No atomics, no arrival counters, no waiting on memory, no assumption that
 * workgroups are co-resident; capturable into a graph; no allocation, no synchronisation.
 * workspace_dev: smc_gbm_price_sliced_workspace_bytes bytes = 8 n_contracts (6 W + 1), 8-byte aligned: partials
 * [B][W][6], then totals [B].  It needs no zeroing (every slot read was written earlier in the same call) and holds
 * nothing between calls.
 * Checks, in this order, all before the empty batch (n_contracts = 0: SMC_OK, nothing touched) is accepted:
 * smc_gbm_price's (NULL contracts_dev: SMC_ERR_INVALID_ARGUMENT; n_contracts < 0 or >= 2^31, timesteps <= 0,
 * n_paths <= 0 or >= 2^40: SMC_ERR_INVALID_SHAPE; dtype, NULL prices_dev, bad scheme or unknown flag, SMC_MATH_REF,
 * SMC_MATH_HW with f64, bad normalization: SMC_ERR_INVALID_ARGUMENT); SMC_PRICE_REPLAY or SMC_TRAIN_DYNAMIC:
 * SMC_ERR_INVALID_ARGUMENT (there is no mode to force); slice_paths <= 0 or not a multiple of 2048:
 * SMC_ERR_INVALID_SHAPE; W > 65,535 or n_contracts W >= 2^31: SMC_ERR_INVALID_SHAPE; NULL workspace_dev or
 * workspace_bytes below the query: SMC_ERR_INVALID_ARGUMENT.
 * Out of scope: sliced path-dependent or basket pricing (the same pattern with more partials; the workspace layout
 * [B][W][k] and the slice rule are meant to carry over, as they did to smc_gbm_greeks_sliced below); parking slices
 * to save the NORMALIZE replay; a slice length chosen from the batch size. */
int32_t smc_gbm_price_sliced(const double* contracts_dev /*[B][6]*/, int64_t n_contracts, int32_t timesteps,
                             int64_t n_paths, int64_t slice_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                             int64_t ordinal0, int32_t scheme, int32_t normalization, int32_t dtype,
                             double* prices_dev /*[B][8]*/, void* workspace_dev, int64_t workspace_bytes,
                             void* stream);
/* 8 n_contracts (6 W + 1); -1 for arguments the call rejects (n_contracts < 0 or >= 2^31, n_paths <= 0 or >= 2^40,
 * slice_paths <= 0 or not a multiple of 2048, W > 65,535, n_contracts W >= 2^31). */
int64_t     smc_gbm_price_sliced_workspace_bytes(int64_t n_contracts, int64_t n_paths, int64_t slice_paths);
/* The default slice length, from n_paths alone: 2048 max(1, ceil(n_paths / (2048 x 512))), 512 being two workgroups
 * on each of 256 CUs; so the block a default call gives does not change with the batch size or the device.  -1 for
 * n_paths <= 0 or >= 2^40. */
int64_t     smc_gbm_price_slice_paths(int64_t n_paths);
/* "price_slice_kernel(raw)", "price_slice_kernel(replay)" or "unsupported" (a shape, scheme, normalization or dtype
 * the call rejects).  Static string, no device call. */
const char* smc_gbm_price_sliced_kernel(int32_t timesteps, int64_t n_paths, int64_t slice_paths, int32_t scheme,
                                        int32_t normalization, int32_t dtype);

/* ---- sliced batched Greeks: one contract's Greeks across workgroups (additive under ABI 21) -----
 * smc_gbm_greeks' 26 columns (SMC_GREEKS_COLS: the same per-path table, constants and conventions for v = 0, T = 0
 * and n_paths = 1) in smc_gbm_price_sliced's geometry: W = ceil(n_paths / slice_paths) slices of slice_paths paths (a
 * positive multiple of 2048; the last slice is ragged and ends at n_paths), workgroup b W + w for slice w of contract
 * b, the streams (seed, ordinal, p0 / 4, timesteps) with the contract-global p0; lanes wholly past the slice end
 * neither draw nor contribute.  Log-Euler only, SMC_MATH_HW f32 only.  The default slice length is
 * smc_gbm_price_slice_paths(n_paths): there is no second rule, so a price and its Greeks are cut identically.
 * Order.  Inside a slice, smc_gbm_greeks' order over the slice's own chunks (per lane over the chunks ascending, the
 * wave butterfly xor 32..1, waves 0..7).  A workgroup leaves up to 22 f64 partials in the workspace: the 20 sums of
 * the ten per-path terms and their squares, the raw terminal sum (the lane's 4 values summed in the sim dtype first)
 * and, under SMC_NORM_NORMALIZE, sum f64(x L).  Each total of a contract is slice 0's value, then + slice 1, ...,
 * + slice W - 1 (greeks_finish_kernel, one thread per total); the columns are smc_gbm_greeks' closing arithmetic on
 * the totals: mean and standard error per term, gamma and its error from vega over v T X0^2 in f64, columns 24 / 25
 * the total raw sum / sum x L (column 25 is 0 under SMC_NORM_RAW).  Under SMC_NORM_NORMALIZE the payoff scale and the
 * constants of the weights come from the contract's two totals, exactly as smc_gbm_greeks takes them from its sums.
 * Promises.  The block is bit-identical run to run, under any split of the batch, and whatever the workspace held.
 * For slice_paths >= n_paths (W = 1) it is smc_gbm_greeks | SMC_PRICE_REPLAY's bit for bit (under SMC_NORM_RAW:
 * greeks_kernel(raw)'s).  At any W, columns 20, 21, 22, 23, 24 are smc_gbm_price_sliced's columns 0, 1, 3, 4, 7 at the
 * same slice_paths, bit for bit (the same per-path values in the same order).  At W > 1 the other columns may differ
 * from smc_gbm_greeks' in their last bits only: the f64 sums are associated by slice.
 * Launches, in stream order on `stream`: SMC_NORM_RAW two (greeks_slice_kernel: the raw sum and the 20 sums at scale
 * 1; greeks_finish_kernel); SMC_NORM_NORMALIZE four (greeks_slice_kernel for the two sums; greeks_finish_kernel for
 * the totals; greeks_slice_kernel again, replaying its slice's streams; greeks_finish_kernel for the columns).  No
 * atomics, no arrival counters, no waiting on memory, no assumption that workgroups are co-resident; capturable into
 * a graph; no allocation, no synchronisation; no parked mode.
 * workspace_dev: smc_gbm_greeks_sliced_workspace_bytes bytes = 8 n_contracts (22 W + 2), 8-byte aligned: partials
 * [B][W][22], then totals [B][2].  It needs no zeroing (every slot read was written earlier in the same call) and
 * holds nothing between calls.
 * Checks, in this order, all before the empty batch (n_contracts = 0: SMC_OK, nothing touched) is accepted:
 * smc_gbm_greeks' (NULL contracts_dev: SMC_ERR_INVALID_ARGUMENT; n_contracts < 0 or >= 2^31, timesteps <= 0,
 * n_paths <= 0 or >= 2^40: SMC_ERR_INVALID_SHAPE; dtype, NULL greeks_dev, bad scheme or unknown flag, SMC_MATH_REF,
 * SMC_MATH_HW with f64, bad normalization, SMC_SCHEME_SIMPLE_EULER: SMC_ERR_INVALID_ARGUMENT); SMC_PRICE_REPLAY or
 * SMC_TRAIN_DYNAMIC: SMC_ERR_INVALID_ARGUMENT (there is no mode to force); then smc_gbm_price_sliced's slice_paths,
 * W <= 65,535, n_contracts W < 2^31 and workspace checks, with its codes.
 * Out of scope: sliced Greeks of the path-dependent or basket payoffs; parking slices; simple Euler. */
int32_t smc_gbm_greeks_sliced(const double* contracts_dev /*[B][6]*/, int64_t n_contracts, int32_t timesteps,
                              int64_t n_paths, int64_t slice_paths, uint64_t mc_seed, const int64_t* ordinal_dev,
                              int64_t ordinal0, int32_t scheme, int32_t normalization, int32_t dtype,
                              double* greeks_dev /*[B][26]*/, void* workspace_dev, int64_t workspace_bytes,
                              void* stream);
/* 8 n_contracts (22 W + 2); -1 for the arguments smc_gbm_price_sliced_workspace_bytes rejects. */
int64_t     smc_gbm_greeks_sliced_workspace_bytes(int64_t n_contracts, int64_t n_paths, int64_t slice_paths);
/* "greeks_slice_kernel(raw)", "greeks_slice_kernel(replay)" or "unsupported" (a shape, scheme, normalization or dtype
 * the call rejects).  Static string, no device call. */
const char* smc_gbm_greeks_sliced_kernel(int32_t timesteps, int64_t n_paths, int64_t slice_paths, int32_t scheme,
                                         int32_t normalization, int32_t dtype);

#ifdef __cplusplus
}
#endif

#endif /* SPECTRALMC_HIP_H */
