/*
 * ocx.h — C ABI of the MI355X online-convex-optimization engine (libocx.so).
 *
 * Drop-in boundary for the reference's per-timestep FTRL/FTL hot path
 * (revvu/online_convex_optimization, /root/reference).  The reference is pure
 * Python: its "operator API" is the module-level functions that the drivers
 * select by import (fast_driver.py:23-28 vs driver.py:22-27).  Every entry point
 * below names the reference function it replaces; the ctypes binding a maintainer
 * adds on the reference side is shown in INTEGRATION.md and implemented in
 * online_convex_optimization_amd/_lib.py.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - Every function returns 0 on success or a negative ocx_status; the message
 *     of the last failure on the calling thread is available via ocx_last_error().
 *   - "host" entry points take host (numpy) pointers, copy to device `device`, run
 *     the HIP kernels and copy results back (synchronous).
 *   - "dev" entry points take device pointers in the engine's tiled HBM layout
 *     (see ocx_layout) and a hipStream_t passed as void* (NULL = default stream);
 *     they are asynchronous and capture-safe (no allocation, no sync) — except
 *     ocx_dev_exact_ball_solve / _tiled at d > 64, which take their Newton systems' scratch
 *     stream-ordered (hipMallocAsync / hipFreeAsync on the caller's stream; no sync).
 *   - All arithmetic is IEEE binary64 (dtype "f64").
 *   - lanes_per_seq selects how a sequence's d coordinates map onto lanes:
 *       0      auto: the fewest lanes that fill the GPU; partial sums combined by a
 *              butterfly (~1e-16 relative to the reference's sequential sums);
 *       k >= 2 k lanes (power of two), butterfly sums;
 *       1      exact, auto lanes (<= 16 coordinates per lane, <= 32 from d = 512 on;
 *              <= 4 lanes unless d needs more): every sum in the reference's
 *              sequential order, so results are bit-identical;
 *       -k     exact with k lanes; for k > 1 the running sum is handed from lane to
 *              lane (layout.chain = 1);
 *       OCX_LANES_BEST (128)  the fastest certified mode, the default of the batched
 *              APIs: the exact layout's sums (value 1) wherever its lane chains are short
 *              (fewer than 8 lanes per sequence) and d < 64; butterfly sums otherwise —
 *              d >= 512 and few-wave batches such as the capacity-limited T = 1e5 g(T)
 *              batch, where a chain of 8+ lanes leaves the kernel latency-bound, and
 *              batches of >= 4096 sequences at 64 <= d <= 128, where the pipelined 8 x 8
 *              butterfly kernel beats the 4-lane chain and the generator writes whole
 *              128-B lines of its tile.  The g(T) and FTRL-vs-exact entry points also
 *              take the closed-form comparator losses in this mode wherever the kernel
 *              certifies them (ocx_dev_simulate_alg_ex), so their results are NOT
 *              bit-identical to the reference: the loops keep the sums above, the
 *              comparator loss differs from the reference's sequential sum by that sum's
 *              rounding (about 1e-13 relative on the regret at T = 1e4).  Use 1 (or -k)
 *              for bit-identical results: every drop-in module does.
 */
#ifndef OCX_H_
#define OCX_H_

#define OCX_LANES_BEST 128
/* ocx_version() == OCX_VERSION = 10000 * major + 100 * minor + patch (400 = 0.4.0).  0.2.0:
 * ocx_ftrl_vs_exact_batch has its round-1 signature again (the `norm` argument moved to
 * ocx_ftrl_vs_exact_batch_ex); callers built against 0.1.x check ocx_version() >= 200.
 * 0.3.0 adds the general exact-FTL solver (ocx_exact_ball_solve, ocx_dev_exact_ball_solve,
 * ocx_dev_exact_ball_solve_tiled); nothing existing changed.  0.4.0 adds
 * ocx_dev_gen_simulate (generation overlapped with FTRL); nothing existing changed.
 * The regret-curve symbols (ocx_curve_workspace_bytes, ocx_dev_simulate_alg_curve,
 * ocx_simulate_alg_curve_batch) were added without a version change: the number stays 400 and
 * nothing existing changed; a caller that needs them looks the symbols up.  The same holds for
 * the step-size sweep symbols (ocx_etas_group, ocx_dev_simulate_alg_etas,
 * ocx_simulate_alg_etas_batch) and the threshold sweep symbols (ocx_smart_thresholds_group,
 * ocx_dev_simulate_smart_thresholds, ocx_simulate_smart_thresholds_batch), and for the SMART
 * regret-curve symbols (ocx_smart_curve_group, ocx_dev_simulate_smart_curve,
 * ocx_simulate_smart_curve_batch), and for the FTRL-vs-exact-FTL regret-curve symbols
 * (ocx_ftrl_exact_curve_workspace_bytes, ocx_dev_ftrl_vs_exact_curve,
 * ocx_ftrl_vs_exact_curve_batch), and for the float32 twin's column symbols
 * (ocx_twin32_cols_group, ocx_dev_twin32_cols, ocx_twin32_cols_batch), and for the regret-grid
 * symbols (ocx_curve_etas_group, ocx_curve_etas_workspace_bytes,
 * ocx_dev_simulate_alg_curve_etas, ocx_simulate_alg_curve_etas_batch,
 * ocx_dev_max_regret_cols), and for the SMART regret-grid symbols (ocx_smart_grid_group,
 * ocx_dev_simulate_smart_grid, ocx_simulate_smart_grid_batch), and for the FTRL-vs-exact-FTL
 * regret-grid symbols (ocx_ftrl_exact_grid_group, ocx_ftrl_exact_grid_workspace_bytes,
 * ocx_dev_ftrl_vs_exact_curve_etas, ocx_ftrl_vs_exact_curve_etas_batch), and for the label-bit
 * symbols (ocx_label_bits_words, ocx_dev_pack_bits, ocx_dev_gen_gT_bits,
 * ocx_dev_simulate_alg_bits), and for the anytime-regret symbol
 * (ocx_dev_simulate_alg_anytime).
 *
 * Checking the ABI: one intermediate 0.1.x tree exported ocx_ftrl_vs_exact_batch WITH a
 * `norm` argument under the same symbol and the same version number as the release without
 * it, so a version number alone cannot tell those two apart and a C linker will not either.
 * A C caller must therefore require EXACT equality, ocx_version() == the OCX_VERSION it was
 * compiled with (OCX_ABI_MATCHES() below), not ocx_version() >= some minimum, and must take
 * `norm` through ocx_ftrl_vs_exact_batch_ex only.  The Python binding (_lib.py) checks
 * equality the same way. */
#define OCX_VERSION 400

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ocx_status {
    OCX_OK = 0,
    OCX_E_INVALID = -1,   /* bad argument / shape */
    OCX_E_HIP = -2,       /* HIP runtime error (no device, launch failure, OOM) */
    OCX_E_UNSUPPORTED = -3
} ocx_status;

/* Tiled HBM layout shared by the generators and the simulation kernels.
 * A wave-group is 64 lanes = S sequences x P lanes; lane L = s*P + c owns
 * coordinates [c*C, (c+1)*C) of sequence b = g*S + s.  Coordinate pair k of every
 * lane lives in "plane" k (k < C/2): per (g, t) one contiguous 1 KiB row
 * [lane 0..63][2].  A wave therefore streams C/2 independent contiguous regions
 * (one per plane) with fully coalesced 1 KiB dwordx4 loads, which keeps more HBM
 * streams open than one region per wave:
 *   z_tiled[((k*G + g)*T + t)*128 + L*2 + e] = z[b][t][c*C + 2k + e]
 *   y_tiled[(g*T + t)*S + s]                 = y[b][t]
 * Padding (coordinates j >= d, sequences b >= B) holds zeros.
 *
 * The label-bit tile (optional, beside y_tiled; ocx_label_bits_words(L) 64-bit words, 1/64 of
 * y_tiled): one word per wave-group g, 64-step block k < ceil(T/64) and sequence slot s < S,
 *   y_bits[(g*ceil(T/64) + k)*S + s]  bit (t mod 64)  =  (y[b = g*S + s][64k + (t mod 64)] == +1)
 * with the bits at t >= T and of padding sequences 0.  It stands for y_tiled only where every
 * label of a real sequence is exactly +1 or -1 (the g(T) sampler's are); the pipelined
 * FTRL / FTL step then reads one bit per label instead of one double (ocx_dev_simulate_alg_bits).
 * The layout holds for every P and S. */
typedef struct ocx_layout {
    int64_t B, T, d;  /* logical sizes */
    int32_t P;        /* lanes per sequence (1..64, power of two) */
    int32_t C;        /* coordinates per lane (even) */
    int32_t S;        /* sequences per wave-group = 64 / P */
    int32_t chain;    /* 1: exact mode with P > 1 (running sum passed lane to lane) */
    int64_t Dp;       /* padded dimension P*C >= d */
    int64_t G;        /* wave-groups = ceil(B / S) */
    int64_t z_elems;  /* doubles in z_tiled = G*T*64*C */
    int64_t y_elems;  /* doubles in y_tiled = G*T*S */
} ocx_layout;

/* ---- library / device ---------------------------------------------------- */
int ocx_version(void);
/* 1 when the loaded library implements exactly the ABI this header describes. */
#define OCX_ABI_MATCHES() (ocx_version() == OCX_VERSION)
int ocx_last_error(char* buf, size_t len);
int ocx_device_count(int* count);
/* Free the HBM the library caches per device for its host entry points and g(T) sweeps
 * (grown on demand, kept between calls).  Safe between calls; the next call regrows it.
 * Use before allocating large device buffers of one's own (engine.DeviceBatch). */
int ocx_release_buffers(int device);
/* Fill *out for (B, T, d) and a lanes_per_seq request (see Conventions). */
int ocx_layout_init(int64_t B, int64_t T, int64_t d, int lanes_per_seq, ocx_layout* out);
/* 64-bit words in the layout's label-bit tile: G * ceil(T/64) * S (negative: an error). */
int64_t ocx_label_bits_words(const ocx_layout* L);

/* ---- host entry points (numpy buffers in, results out) ------------------- */

/* fast_algorithms.py:171-177 simulate_alg (→ _simulate_alg_core :88-115), batched
 * over B independent sequences; also exact_ftl.py:230-277 _simulate_ftrl when
 * `comparator` ([B][d], nullable) replaces the final FTL action.
 *   z [B][T][d], y [B][T] (C-contiguous f64); alg_flag 0 = FTRL, else FTL.
 *   regret/cum_loss/comp_loss [B] (each nullable); x_last [B][d] nullable =
 *   the last action played (exact_ftl.py:276). */
int ocx_simulate_alg_batch(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                           int alg_flag, double eta0, const double* comparator, double* regret,
                           double* cum_loss, double* comp_loss, double* x_last,
                           int lanes_per_seq, int device);

/* fast_algorithms.py:184-195 simulate_SMART_like (→ :118-164), batched; thresh [B].
 * switch_step [B] nullable: the t at which the switch fired, or -1.  In the bit-exact modes
 * (lanes_per_seq 1 or -k) the reference's O(T²·d) prefix re-scan and streamed comparator;
 * otherwise the O(T·d) kernel of ocx_dev_simulate_smart_ex with both flags (the same
 * switch steps; the comparator loss within its rounding). */
int ocx_simulate_smart_batch(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                             const double* thresh, double eta0, double* regret,
                             int64_t* switch_step, int lanes_per_seq, int device);

/* exact_ftl.py:423-453 run_ftl_exact (compute_prefix_actions :280-303 + replay
 * :306-333) over the unit ball of `norm` (0 l2, 1 l1, 2 linf; ExactFTLNoClip :83-105),
 * batched, in the closed form that is exact when every row's dual norm is <= 1 and
 * y_t = ±1 (then |z_i·x| <= 1 on the ball and ½Σ|z_i·x − y_i| = ½(t − x·S_t),
 * S_t = Σ_{i<t} y_i z_i): the prefix minimiser maximises x·S_t over the ball:
 *   l2   S_t/||S_t|| (0 if S_t = 0)            regime ||z_t||_2^2 <= 1 + 1e-6
 *   l1   sign(S_j*) e_j*, j* = first argmax |S_j|  regime max_j |z_tj| <= 1 + 1e-12
 *   linf sign(S_t) componentwise (0 where S_tj = 0)  regime sum_j |z_tj| <= 1 + 1e-12
 * regime [B] (int32, 1 = the data were in that regime); outside it the returned numbers
 * are not the SOCP/LP solution and callers must reject them.  Where the maximiser is not
 * unique (S_t = 0, ties in |S_j|, zero coordinates under linf) the solver's choice is
 * arbitrary; the engine returns the point above.  cmp_action [B][d] nullable = actions[T]
 * (the exact comparator of the whole sequence).  The reference solves an SOCP / LP with
 * cvxpy, absent here: parity unpinned, validated against scipy's solvers. */
int ocx_ftl_exact_batch(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                        int norm, double* cum_loss, double* comp_loss, double* cmp_action,
                        int32_t* regime, int lanes_per_seq, int device);

/* exact_ftl.py:280-303 compute_prefix_actions (ExactFTLNoClip, `norm` as above), batched:
 * actions [B][T+1][d] row-major, actions[b][t] = the exact FTL solution of prefix length
 * t, in the closed form of ocx_ftl_exact_batch (S_t/||S_t||, 0 for S_t = 0), with the
 * same regime flags (int32 [B], required).  Replaying these actions (ocx_replay_batch)
 * gives ocx_ftl_exact_batch's cum_loss bit for bit.  Parity vs cvxpy: unpinned. */
int ocx_ftl_prefix_actions_batch(const double* z, const double* y, int64_t B, int64_t T,
                                 int64_t d, int norm, double* actions, int32_t* regime,
                                 int lanes_per_seq, int device);

/* exact_ftl_driver.py:157-186 per sequence, batched, in one read of the data: exact FTL
 * (as ocx_ftl_exact_batch over the `norm` ball) and FTRL (fast_algorithms.py:88-111 order,
 * eta0) against the exact comparator actions[T] (exact_ftl.py:399-420 run_ftrl with
 * comparator_action).  Outputs [B]: cum_ftrl, cum_exact, comp_exact (the loss of
 * actions[T], shared by both regrets: FTRL = cum_ftrl - comp_exact, exact FTL =
 * cum_exact - comp_exact), comp_ftl (nullable: the loss of FTL(theta_ftrl), the
 * comparator simulate_alg itself would use), cmp_action [B][d] (nullable) and regime
 * (int32, required; see ocx_ftl_exact_batch). */
int ocx_ftrl_vs_exact_batch(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                            double eta0, double* cum_ftrl, double* cum_exact, double* comp_exact,
                            double* comp_ftl, double* cmp_action, int32_t* regime,
                            int lanes_per_seq, int device);
/* ocx_ftrl_vs_exact_batch over the unit ball of `norm` (0 l2 — what the plain entry point
 * uses —, 1 l1, 2 linf), as ocx_ftl_exact_batch.  (Version 200 restored the plain entry
 * point's round-1 signature; `norm` lives here.) */
int ocx_ftrl_vs_exact_batch_ex(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                               double eta0, double* cum_ftrl, double* cum_exact,
                               double* comp_exact, double* comp_ftl, double* cmp_action,
                               int32_t* regime, int norm, int lanes_per_seq, int device);

/* The general exact-FTL comparator: ExactFTLNoClip's problem (exact_ftl.py:83-105,
 * solved with cvxpy at :119-128)
 *     min_x ½ Σ_{i<n} |z_i·x − y_i|   s.t.  ||x||_norm <= 1   (norm 0 l2, 1 l1, 2 linf)
 * for any rows and labels (no regime: where the closed forms above do not apply), on device
 * by a primal log-barrier path (damped Newton, μ from 1 to 1e-10), then a
 * polish: the active rows and face found at several thresholds, x purified onto them and the
 * dual rebuilt from the KKT system.  The path's own x is kept whenever the barrier's dual or
 * a rebuilt one certifies it (gap <= 1e-9·(1 + obj)); the purified x replaces it only where x
 * alone does not certify and the purified point tightens the certificate.  Where the
 * minimiser is not unique the path aims at its limit, the analytic centre of the optimal
 * face.  Asserted by tests/test_gpu_exact_centre.py: within 1e-6 of that
 * centre on most faces tested and within 7e-6 on all of them at d <= 256 (ties, interpolation
 * faces of prefixes n < d), except where x does not certify alone and is purified — seen on
 * one near-vertex l1 face at d = 256, where the face's vertex 5.7e-5 away is returned.
 * Problems: each sequence's prefixes n = 0..T (all_prefixes = 1, actions
 * [B][T+1][d] as compute_prefix_actions :280-303 returns; actions[b][0] = 0) or n = T only
 * (all_prefixes = 0, [B][1][d]: the comparator).  obj [B][NP] (nullable) = ½Σ|r| at x
 * (for n = T: the comparator loss, exact_ftl.py:224-227, in butterfly order); gap [B][NP]
 * (nullable) = obj minus a dual lower bound (a certificate: obj − optimum <= gap);
 * step_loss [B][NP] (nullable) = ½|z_n·x_n − y_n|, what FTL pays at step n with the prefix-n
 * action (replay_exact_ftl :318-323; 0 for n = T), so Σ_n step_loss is exact FTL's cumulative
 * loss; info [B][NP] (int32, nullable) = the solve's status and Newton steps:
 *   info >= 0, bit OCX_EXACT_INFO_BREAKDOWN clear: converged (steps; 0: the empty prefix);
 *   info < 0: the step cap (300 steps; 1000 for d > 64) ended the solve (-steps);
 *   bit OCX_EXACT_INFO_BREAKDOWN set: stopped where μ outran fp64 (a Newton decrement no
 *     centred step produces) at the last centre, after (info & 0xFFFFF) steps — accurate to
 *     that μ only.
 * Only a converged solve is an answer by itself; for the other two the certificate decides
 * (the engine accepts a solve iff info >= 0 and gap <= 1e-8·(1 + |obj|), and raises
 * otherwise, as exact_ftl.py:125-126 does on a solver failure).  1 <= d <=
 * OCX_EXACT_BALL_MAX_D (else OCX_E_UNSUPPORTED).  Parity vs cvxpy: unpinned (validated
 * against scipy's HiGHS LPs and by the certificate). */
#define OCX_EXACT_INFO_BREAKDOWN (1 << 20)
#define OCX_EXACT_BALL_MAX_D 256
int ocx_exact_ball_solve(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                         int norm, int all_prefixes, double* actions, double* obj, double* gap,
                         double* step_loss, int32_t* info, int device);

/* exact_ftl.py:306-333 replay_exact_ftl, batched: actions [B][T+1][d].
 * cum_loss = sum_{t<T} 0.5|z_t.a_t - y_t|; comp_loss = sum_t 0.5|z_t.a_T - y_t|. */
int ocx_replay_batch(const double* z, const double* y, const double* actions, int64_t B,
                     int64_t T, int64_t d, double* cum_loss, double* comp_loss, int device);

/* fast_algorithms.py:230-241 (the body of empirical_worst_case_thresholds for one T):
 * regenerates on device the R sequences _rng(base_seed, T, run0 + r), r < R, with
 * `d` coordinates (the reference hard-codes d = 5), runs FTRL(eta0) on each and
 * returns the R regrets (host array).  Only the regrets leave the GPU. */
int ocx_gT_regrets(uint64_t base_seed, int64_t T, int64_t run0, int64_t R, int64_t d,
                   double eta0, double* regrets, int lanes_per_seq, int device);
/* ocx_gT_regrets with the regrets written to device memory: regrets_dev [R] lives on
 * `device`.  Nothing crosses PCIe (the FTRL kernel writes each batch's regrets in place);
 * the call returns when they are complete, so any stream or collective (an RCCL all-gather
 * of every rank's shard, parallel.gT_sweep_distributed) may read them afterwards. */
int ocx_gT_regrets_dev(uint64_t base_seed, int64_t T, int64_t run0, int64_t R, int64_t d,
                       double eta0, double* regrets_dev, int lanes_per_seq, int device);
/* ocx_gT_regrets reduced on device: *gmax = max(0.0, max over the R regrets) as
 * fast_algorithms.py:228, :242-243 (bit-identical to the max of ocx_gT_regrets' output);
 * only 8 bytes leave the GPU.  What empirical_worst_case_thresholds needs per T. */
int ocx_gT_max(uint64_t base_seed, int64_t T, int64_t run0, int64_t R, int64_t d, double eta0,
               int lanes_per_seq, int device, double* gmax);
/* In the bit-exact modes (lanes_per_seq 1 or -k) the comparator pass is the reference's
 * sequential sum; in the others the closed form of ocx_dev_simulate_alg_ex applies where
 * the kernel certifies it (the sampler's rows satisfy it by construction). */

/* fast_algorithms.py:211-247 empirical_worst_case_thresholds with `d` coordinates, over
 * several GPUs of this process: for every T of T_grid [nT], the runs [0, runs) are split
 * into contiguous shards, one per device, each generated and simulated on its own GPU by a
 * host thread (ocx_gT_regrets).  gmax [nT] = max(0.0, max over runs) as :228,:242-243;
 * regrets [nT][runs] (nullable: then each shard's max is reduced on its GPU, ocx_gT_max)
 * in run order.  ngpus <= 0: every visible device. */
int ocx_gT_sweep(const int64_t* T_grid, int nT, int64_t runs, uint64_t base_seed, int64_t d,
                 double eta0, int ngpus, double* gmax, double* regrets);
/* ocx_gT_sweep over an explicit device list (a device may repeat: its shards then share
 * that device's stream) and a lanes_per_seq mode. */
int ocx_gT_sweep_devices(const int64_t* T_grid, int nT, int64_t runs, uint64_t base_seed,
                         int64_t d, double eta0, const int* devices, int ndev, int lanes_per_seq,
                         double* gmax, double* regrets);

/* exact_ftl.py:224-227 `_comparator_loss` (0.5 * sum |z @ x - y|) for B sequences in the
 * reference's own operation order: OpenBLAS dgemv_t's row sums and NumPy's pairwise sum
 * (DESIGN.md §4).  z [B][T][d], y [B][T] row-major, x [B][d] the comparator actions.
 * The exact_ftl drop-in uses it for every RunResult.comp_loss. */
int ocx_comparator_loss_blas_batch(const double* z, const double* y, const double* x, int64_t B,
                                   int64_t T, int64_t d, double* comp_loss, int device);

/* ---- float32 twin (algorithms.py, the module driver.py imports) ----------- */
/* algorithms.py:28-54 simulate_alg (algo 0 FTRL, 1 FTL) and :65-120 simulate_SMART_like
 * (algo 2, thresh[B] = theta_thresh per sequence), batched over B sequences of float32 rows
 * z[B][T][d], y[B][T], d <= 32, in NumPy 2's float32 arithmetic:
 * result[b] = the twin's np.float32 return value; cum_loss (double, the Python float
 * accumulator), comp_loss (float32) and switch_step (SMART: step of the switch, -1 if none)
 * are optional. */
int ocx_twin32_batch(const float* z, const float* y, int64_t B, int64_t T, int64_t d, int algo,
                     double eta0, const double* thresh, float* result, double* cum_loss,
                     float* comp_loss, int64_t* switch_step, int device);
/* ocx_twin32_batch on a device-resident batch in a one-lane layout (lanes_per_seq = -1);
 * thresh (SMART) is a device array [B]; result / comp_loss are float32. */
int ocx_dev_twin32(const ocx_layout* L, const double* z_tiled, const double* y_tiled, int algo,
                   double eta0, const double* thresh, float* result, double* cum_loss,
                   float* comp_loss, int64_t* switch_step, void* stream);
/* Twin sweeps: the float32 twin for K columns (horizon t_k, algorithm, threshold) per staging
 * of a sequence's rows and per prefix re-scan (one wavefront per sequence).
 * Column k carries the bits of ocx_dev_twin32(algos[k], eta0, thresh[:, k]) on a batch made of
 * the first horizons[k] rows:
 *   result[b][k] float32, cum_loss[b][k] double, comp_loss[b][k] float32, switch_step[b][k]
 *   int64 (-1: never switched, and every FTRL / FTL column).
 * horizons [K]: non-decreasing in [0, T], duplicates legal (FTRL, FTL, SMART and EMP at the
 * same t_k); a horizon of 0 gives 0.0f, 0.0, 0.0f, -1.  algos [K]: 0 FTRL, 1 FTL, 2 SMART.
 * eta0: one scalar per call.  SMART's pre-switch prefix loss at step t is the comparator loss
 * of a run truncated at t + 1 and FTL is the SMART column that never switches, so one re-scan
 * per step decides every column; a launch serves a group of consecutive columns and stops at
 * the group's last horizon.  The rows of the call's last horizon must fit the LDS,
 * t_K * (C + 1) * 4 <= 60 KiB (C = d rounded up to even: 2194 rows at d = 5); otherwise
 * OCX_E_UNSUPPORTED before anything is launched (no lane-per-sequence form, no clip variant).
 *
 * columns one launch serves in layout L (the smallest of 1, 2, 4, 8 that holds K, at most
 * 8 for d <= 8, 4 for d <= 16, 2 for d <= 32; negative ocx_status on error) */
int ocx_twin32_cols_group(const ocx_layout* L, int64_t K);
/* device: one-lane layout (lanes_per_seq = -1), as ocx_dev_twin32.  horizons and algos are
 * HOST arrays [K], read and validated at call time (they travel in the kernel arguments): a
 * bad list (order, range, algorithm, a SMART column with thresh == NULL) returns
 * OCX_E_INVALID and nothing is launched.  thresh: DEVICE [B][K] row-major, read for SMART
 * columns only, NULL allowed when no column is SMART.  result [B][K] device; cum_loss,
 * comp_loss, switch_step [B][K] device, each nullable.  K == 0, B == 0 and T == 0 are valid.
 * Asynchronous, no allocation, no copy, no sync: capture-safe like the other dev entry points
 * (a captured graph keeps the lists it was captured with). */
int ocx_dev_twin32_cols(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                        int64_t K, const int64_t* horizons, const int32_t* algos, double eta0,
                        const double* thresh, float* result, double* cum_loss, float* comp_loss,
                        int64_t* switch_step, void* stream);
/* host: float32 z [B][T][d], y [B][T] in, [B][K] out (thresh HOST [B][K], nullable when no
 * column is SMART; the last three outputs nullable), on the library's cached buffers like
 * ocx_twin32_batch; the lists are validated before any device is touched. */
int ocx_twin32_cols_batch(const float* z, const float* y, int64_t B, int64_t T, int64_t d,
                          int64_t K, const int64_t* horizons, const int32_t* algos, double eta0,
                          const double* thresh, float* result, double* cum_loss, float* comp_loss,
                          int64_t* switch_step, int device);
/* The float32 twin's g(T) inner loop (algorithms.py:150-169): the regrets of runs
 * run0 .. run0+R-1 of _rng(base_seed, T, run), rows rounded to float32 and clipped in
 * float32, FTRL with eta0; on device (generator + twin kernel), nothing but the regrets
 * crosses PCIe. */
int ocx_twin32_gT_regrets(uint64_t base_seed, int64_t T, int64_t run0, int64_t R, int64_t d,
                          double eta0, float* regrets, int device);

/* ---- device entry points (tiled layout, caller-owned device memory) ------ */

/* Re-tile device arrays z [B][T][d], y [B][T] into the layout. */
int ocx_dev_pack(const ocx_layout* L, const double* z, const double* y, double* z_tiled,
                 double* y_tiled, void* stream);

/* ocx_dev_pack that also writes the label-bit tile y_bits (device, ocx_label_bits_words(L)
 * words) and *not_unit (device int32): 1 if any label of a real sequence is not exactly +1 or
 * -1 — y_bits must then not be used — else 0. */
int ocx_dev_pack_bits(const ocx_layout* L, const double* z, const double* y, double* z_tiled,
                      double* y_tiled, uint64_t* y_bits, int32_t* not_unit, void* stream);

/* fast_algorithms.py:231-239 sampler on device: sequence b of the layout is
 * _rng(base_seed, T, run0 + b) → clipped N(0, I_d) rows and ±1 labels. */
int ocx_dev_gen_gT(const ocx_layout* L, uint64_t base_seed, int64_t run0, double* z_tiled,
                   double* y_tiled, void* stream);
/* ocx_dev_gen_gT that also fills the label-bit tile y_bits (nullable: ocx_dev_gen_gT); z_tiled
 * and y_tiled are written exactly as by ocx_dev_gen_gT. */
int ocx_dev_gen_gT_bits(const ocx_layout* L, uint64_t base_seed, int64_t run0, double* z_tiled,
                        double* y_tiled, uint64_t* y_bits, void* stream);

/* sequence_generation.py families on device, sequence b of the layout:
 *   family 1  make_random_iid_stream (:54-69): _rng(run_seeds[b], T, stream_ids[b]),
 *             u from _rng(run_seeds[b], 0, 11); fp32 rows, y = sign(z.u) (0 → +1);
 *   family 2  make_noisy_iid_stream (:72-89): u from stream 21, labels flipped where
 *             gen.random(T) < p;
 *   family 3  flip_sequence (:24-28);  family 4  switching_two_leaders_sequence
 *             (:36-47) with block_len.  Families 3/4 ignore the seed arrays.
 * run_seeds / stream_ids are device uint64 [B].  The float32 rows are stored as the
 * float64 values simulate_alg's np.ascontiguousarray(z, float64) would see. */
int ocx_dev_gen_family(const ocx_layout* L, int family, const uint64_t* run_seeds,
                       const uint64_t* stream_ids, double p, int64_t block_len, double* z_tiled,
                       double* y_tiled, void* stream);

/* fast_algorithms.py:88-115 on device.  comparator [B][d] device, nullable.
 * Outputs are device arrays [B] (nullable) and x_last [B][d] (nullable). */
int ocx_dev_simulate_alg(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                         int alg_flag, double eta0, const double* comparator, double* regret,
                         double* cum_loss, double* comp_loss, double* x_last, void* stream);

/* ocx_dev_simulate_alg with options.  flags (bitwise or):
 *   OCX_ALG_CLIPPED_ROWS (or its synonym OCX_ALG_CLOSED_COMPARATOR)  closed-form comparator
 *     loss where the kernel certifies it.  With comparator == NULL, the loss of
 *     FTL(theta_T) over the sequence is T/2 - ||theta_T|| whenever every row is inside the
 *     unit ball (||z_t||^2 <= 1 + 1e-12, as the g(T) sampler's clipped rows are,
 *     fast_algorithms.py:234-237) and every step's sub-gradient was -y_t/2 (y_t = +-1, no
 *     exact tie), because |z_t.x* - y_t| = 1 - y_t z_t.x* on the unit ball and
 *     theta_T = -S_T/2.  The kernel checks BOTH conditions itself, row by row and step by
 *     step, for every sequence: the flag is a request, never a trusted assertion, and is
 *     safe on any data.  A wave whose sequences all pass skips the second pass over z: one
 *     HBM pass instead of two.  The comparator loss then equals the reference's sequential
 *     sum up to that sum's rounding (about 1e-12 relative on the regret at T = 1e4; the
 *     loop itself keeps the layout's summation order); a sequence failing the check gets
 *     the streamed second pass, bit-identical to flags 0.
 * closed_out [B] (int32, nullable): 1 where the closed form was taken. */
#define OCX_ALG_CLIPPED_ROWS 1
int ocx_dev_simulate_alg_ex(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                            int alg_flag, double eta0, const double* comparator, double* regret,
                            double* cum_loss, double* comp_loss, double* x_last, int flags,
                            int32_t* closed_out, void* stream);
/* ocx_dev_simulate_alg_ex with the label-bit tile: y_bits (device, nullable) must hold the bits
 * of y_tiled's labels, all of a real sequence's exactly +-1 (ocx_dev_gen_gT_bits, or
 * ocx_dev_pack_bits with *not_unit == 0).  Where the launch is the instance of the pipelined step
 * built for it (the persistent 8 x 8 instance: a d = 64 batch of more wave-groups than are
 * resident at once) the kernel reads the bits instead of y_tiled's doubles, 512.125 instead of
 * 520 bytes per time step (measured: 512.17); every
 * other launch, and y_bits == NULL, is ocx_dev_simulate_alg_ex.  y_tiled is required either way.
 * Same results bit for bit.  OCX_LABEL_BITS=0 in the environment keeps every launch on y_tiled. */
int ocx_dev_simulate_alg_bits(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                              const uint64_t* y_bits, int alg_flag, double eta0,
                              const double* comparator, double* regret, double* cum_loss,
                              double* comp_loss, double* x_last, int flags, int32_t* closed_out,
                              void* stream);

/* Regret curves: fast_algorithms.py:88-115 observed at K checkpoint horizons in one pass.
 * FTRL and FTL are online, so the first t steps of a run on (z, y) are the run on
 * (z[:t], y[:t]): for checkpoints 0 <= t_1 < ... < t_K <= T (strictly increasing; 0 and T
 * allowed) and sequence b,
 *   regret[b][k], cum_loss[b][k], comp_loss[b][k]
 *       == simulate_alg on (z[b][:t_k], y[b][:t_k], alg_flag, eta0)
 * (cum_loss: the loss paid in steps 0 .. t_k - 1; comp_loss: the loss of FTL(theta_{t_k}) over
 * those t_k rows, fast_algorithms.py:113-115 on the prefix; t_k = 0 gives zeros), with the bits
 * ocx_dev_simulate_alg_ex gives on the truncated input in the same layout and with the same
 * flags.  alg_flag 0 = FTRL, else FTL; no caller comparator.
 *
 * bytes of caller-owned device workspace for K checkpoints in layout L
 * (0 for K == 0; negative ocx_status on error) */
int64_t ocx_curve_workspace_bytes(const ocx_layout* L, int64_t K);

/* device: checkpoints is a DEVICE int64 array [K], strictly increasing in [0, L->T] — a
 * precondition the call cannot see: an array that breaks it gives meaningless numbers, but
 * the kernels never leave the batch, the outputs and the workspace whatever it holds;
 * regret / cum_loss / comp_loss: device [B][K] row-major, each nullable;
 * closed_out [B][K] int32 nullable (1 = closed form taken);
 * flags: 0, or OCX_ALG_CLOSED_COMPARATOR / OCX_ALG_CLIPPED_ROWS (one request, as in
 * ocx_dev_simulate_alg_ex: the kernel certifies rows and sub-gradients itself, per prefix;
 * a pair (b, k) it cannot certify gets the streamed pass over its prefix, bit-identical to
 * flags 0, and a certified sequence keeps the closed form whatever shares its wave);
 * workspace: workspace_bytes >= ocx_curve_workspace_bytes(L, K) of device memory, 8-byte
 * aligned, the call's own until the stream has passed it;
 * K == 0, B == 0 and T == 0 are valid and launch nothing or next to nothing;
 * asynchronous, no allocation, no sync: capture-safe like the other dev entry points.
 * Cost: one read of z when every prefix is certified; otherwise the prefixes of the
 * uncertified pairs are read once more (at most sum_k t_k rows per sequence). */
int ocx_dev_simulate_alg_curve(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                               int alg_flag, double eta0, const int64_t* checkpoints, int64_t K,
                               double* regret, double* cum_loss, double* comp_loss,
                               int32_t* closed_out, int flags, void* workspace,
                               size_t workspace_bytes, void* stream);

/* host: numpy buffers in, [B][K] out; checkpoints is a HOST array, validated here (order,
 * range, K >= 0) before any device is touched.
 * Bit-exact layouts (lanes_per_seq 1 / -k): streamed comparator for every pair;
 * other modes: closed form where certified. */
int ocx_simulate_alg_curve_batch(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                                 int alg_flag, double eta0, const int64_t* checkpoints, int64_t K,
                                 double* regret, double* cum_loss, double* comp_loss,
                                 int32_t* closed_out, int lanes_per_seq, int device);

/* Anytime regret: the running max of the regret over EVERY prefix, in one pass and without a
 * workspace.  With R_t = regret of simulate_alg on (z[b][:t], y[b][:t], alg_flag, eta0) in its
 * closed form cum_t - (t/2 - ||theta_t||) (column t of ocx_dev_simulate_alg_curve with the
 * closed-form flag, bit for bit in the same layout), for t = 1 .. T:
 *   open_from[b]  the first t whose prefix the kernel could not certify (rows in the unit ball,
 *                 labels +-1, sub-gradients -y/2: ocx_dev_simulate_alg_ex's certificate);
 *                 T + 1 if every prefix is certified.  Nothing from open_from[b] on enters the
 *                 other outputs: the caller completes those prefixes with the curve entry
 *   sup[b][k]     max of R_t over 1 <= t <= min(t_k, open_from[b] - 1); -inf if that is empty
 *   argsup[b][k]  the smallest t attaining sup[b][k]; 0 with -inf
 *   trace_tiled   R_t of sequence b = g * S + s at [(g * T + (t - 1)) * S + s] (y_tiled's
 *                 layout, L->y_elems doubles); NaN from open_from[b] on
 * device: checkpoints is a DEVICE int64 array [K], strictly increasing in [1, L->T] — a
 * precondition the call cannot see (K <= T it can): an array that breaks it gives meaningless
 * numbers, but the kernel never leaves the batch and the outputs whatever it holds;
 * sup [B][K] double, argsup [B][K] int64, open_from [B] int64, trace_tiled: each nullable;
 * padding sequences' trace slots are not written;
 * flags: must contain OCX_ALG_CLOSED_COMPARATOR / OCX_ALG_CLIPPED_ROWS (one request): without
 * the closed form the statistic has no one-pass form, and the call returns OCX_E_INVALID;
 * K == 0 without a trace, B == 0 and T == 0 are valid and launch nothing;
 * asynchronous, no allocation, no sync, no workspace: capture-safe like the other dev entry
 * points.  Cost: one read of z, plus one norm of theta per step. */
int ocx_dev_simulate_alg_anytime(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                                 int alg_flag, double eta0, const int64_t* checkpoints, int64_t K,
                                 double* sup, int64_t* argsup, int64_t* open_from,
                                 double* trace_tiled, int flags, void* stream);

/* Step-size sweeps: FTRL (fast_algorithms.py:88-115, alg_flag 0) for M values of eta0 in
 * passes over z that each serve a group of them.  For every m,
 *   regret[b][m], cum_loss[b][m], comp_loss[b][m], closed_out[b][m]
 * are bit for bit what ocx_dev_simulate_alg_ex gives with alg_flag 0, eta0 = etas[m],
 * comparator = x_last = NULL, the same layout and the same flags; they do not depend on the
 * group size in use.  FTRL only (FTL has no step size); no caller comparator, no x_last.
 * etas: any values, any order, duplicates allowed (equal values give equal columns).
 *
 * step sizes one pass over z serves in layout L (1: the single-eta form, once per step size;
 * negative ocx_status on error).  Above 1 only where that group measured faster than M
 * single-eta passes; never above the smallest group that holds M. */
int ocx_etas_group(const ocx_layout* L, int64_t M);

/* device: etas is a HOST array [M], read at call time (it travels in the kernel arguments);
 * regret / cum_loss / comp_loss: device [B][M] row-major, each nullable;
 * closed_out [B][M] int32 nullable (1 = closed form taken);
 * flags: 0, or OCX_ALG_CLOSED_COMPARATOR / OCX_ALG_CLIPPED_ROWS (one request, as in
 * ocx_dev_simulate_alg_ex).  The certificate is per (sequence, eta): the row check is shared,
 * the sub-gradient check is per column; an uncertified pair gets the streamed second pass
 * (z read once per group, not once per column), bit-identical to flags 0, and a certified
 * pair keeps the closed form whatever shares its wave or its group;
 * M == 0, B == 0 and T == 0 are valid (T == 0 gives zeros);
 * asynchronous, no allocation, no sync: capture-safe like the other dev entry points. */
int ocx_dev_simulate_alg_etas(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                              const double* etas, int64_t M, double* regret, double* cum_loss,
                              double* comp_loss, int32_t* closed_out, int flags, void* stream);

/* host: numpy buffers in, [B][M] out; M >= 0 is validated before any device is touched.
 * Bit-exact layouts (lanes_per_seq 1 / -k): streamed comparator for every pair;
 * other modes: closed form where certified. */
int ocx_simulate_alg_etas_batch(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                                const double* etas, int64_t M, double* regret, double* cum_loss,
                                double* comp_loss, int32_t* closed_out, int lanes_per_seq,
                                int device);

/* Regret grids: FTRL (alg_flag 0) for M values of eta0, each observed at K checkpoint horizons,
 * in passes over z that each serve a group of step sizes — the step-size sweep and the regret
 * curve in one call.  For step sizes etas[M] (any values, any order, duplicates allowed) and
 * checkpoints 0 <= t_1 < ... < t_K <= T, the outputs are [B][M][K] row-major and
 *   regret[b][m][k], cum_loss[b][m][k], comp_loss[b][m][k], closed_out[b][m][k]
 * are bit for bit what ocx_dev_simulate_alg_ex gives with alg_flag 0, eta0 = etas[m],
 * comparator = x_last = NULL on (z[b][:t_k], y[b][:t_k]) in the same layout and with the same
 * flags.  So [:, m, :] is ocx_dev_simulate_alg_curve with eta0 = etas[m], and where t_K = T,
 * [:, :, K-1] is ocx_dev_simulate_alg_etas; the result does not depend on the group size in
 * use.  FTRL only (FTL has no step size); no caller comparator, no x_last.
 *
 * step sizes one pass over z serves in layout L (1: one pass per step size; negative
 * ocx_status on error).  ocx_etas_group's rule, less two chained instances that are not
 * compiled, and 2 instead of 4 for the pipelined 8-lane layout at 4 coordinates per lane,
 * where 4 measured slower than 2; every other class of layouts measured the largest group
 * fastest against M curve calls; never above the smallest group that holds
 * M. */
int ocx_curve_etas_group(const ocx_layout* L, int64_t M);

/* bytes of caller-owned device workspace for K checkpoints and M step sizes in layout L:
 * G * K * min(group, M) * 64 * (8 C + 12), one pass's theta, cum and need words, reused by the
 * next group of step sizes on the same stream (0 for K == 0 or M == 0; negative ocx_status on
 * error) */
int64_t ocx_curve_etas_workspace_bytes(const ocx_layout* L, int64_t K, int64_t M);

/* device: etas is a HOST array [M], read at call time (it travels in the kernel arguments);
 * checkpoints is a DEVICE int64 array [K], strictly increasing in [0, L->T] — a precondition
 * the call cannot see: an array that breaks it gives meaningless numbers, but the kernels
 * never leave the batch, the outputs and the workspace whatever it holds;
 * regret / cum_loss / comp_loss: device [B][M][K] row-major, each nullable;
 * closed_out [B][M][K] int32 nullable (1 = closed form taken);
 * flags: 0, or OCX_ALG_CLOSED_COMPARATOR / OCX_ALG_CLIPPED_ROWS (one request, as in
 * ocx_dev_simulate_alg_ex).  The certificate is per (sequence, eta, prefix): the row check is
 * shared across columns, the sub-gradient check is per column, both "so far" at each
 * checkpoint; a triple it cannot certify gets the streamed pass over its own prefix (the
 * rows read once per (wave-group, checkpoint) for all of a pass's columns), bit-identical to
 * flags 0, and a certified triple keeps the closed form whatever shares its wave, its launch
 * or its group;
 * workspace: workspace_bytes >= ocx_curve_etas_workspace_bytes(L, K, M) of device memory,
 * 8-byte aligned, the call's own until the stream has passed it; too small is OCX_E_INVALID
 * and nothing is launched;
 * M == 0, K == 0, B == 0 and T == 0 are valid and launch nothing or next to nothing (t_k = 0
 * gives zeros);
 * asynchronous, no allocation, no sync: capture-safe like the other dev entry points. */
int ocx_dev_simulate_alg_curve_etas(const ocx_layout* L, const double* z_tiled,
                                    const double* y_tiled, const double* etas, int64_t M,
                                    const int64_t* checkpoints, int64_t K, double* regret,
                                    double* cum_loss, double* comp_loss, int32_t* closed_out,
                                    int flags, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* host: numpy buffers in, [B][M][K] out; etas and checkpoints are HOST arrays; M >= 0,
 * K >= 0 and the checkpoints' order and range are validated here before any device is touched.
 * Bit-exact layouts (lanes_per_seq 1 / -k): streamed comparator for every triple;
 * other modes: closed form where certified. */
int ocx_simulate_alg_curve_etas_batch(const double* z, const double* y, int64_t B, int64_t T,
                                      int64_t d, const double* etas, int64_t M,
                                      const int64_t* checkpoints, int64_t K, double* regret,
                                      double* cum_loss, double* comp_loss, int32_t* closed_out,
                                      int lanes_per_seq, int device);

/* column-wise ocx_dev_max_regret: gmax[n] = max(start, max_b regrets[b][n]) over the device
 * array regrets [B][N] row-major, start = +0.0, or with accumulate != 0 what gmax[n] holds (so
 * batches accumulate).  The `reg > max` scan of ocx_dev_max_regret per column: a column of
 * negative regrets gives +0.0 and NaNs are ignored.  gmax: device [N].  Asynchronous. */
int ocx_dev_max_regret_cols(const double* regrets, int64_t B, int64_t N, double* gmax,
                            int accumulate, void* stream);

/* ocx_ftl_exact_batch on device (`norm` 0 l2, 1 l1, 2 linf). */
int ocx_dev_ftl_exact(const ocx_layout* L, const double* z_tiled, const double* y_tiled, int norm,
                      double* cum_loss, double* comp_loss, double* cmp_action, int32_t* regime,
                      void* stream);

/* ocx_ftl_prefix_actions_batch on device: actions [B][T+1][d] row-major (device). */
int ocx_dev_ftl_prefix_actions(const ocx_layout* L, const double* z_tiled,
                               const double* y_tiled, int norm, double* actions,
                               int32_t* regime, void* stream);

/* ocx_ftrl_vs_exact_batch on device: both loops in one pass, both comparator losses in
 * a second (two HBM passes instead of four). */
int ocx_dev_ftrl_vs_exact(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                          double eta0, double* cum_ftrl, double* cum_exact, double* comp_exact,
                          double* comp_ftl, double* cmp_action, int32_t* regime, void* stream);

/* ocx_dev_ftrl_vs_exact with options: `norm` of the exact side (0 l2, 1 l1, 2 linf, as
 * ocx_ftl_exact_batch), and flags OCX_ALG_CLOSED_COMPARATOR (or OCX_ALG_CLIPPED_ROWS):
 * for l2 and every sequence whose rows the kernel finds inside the unit ball
 * (||z_t||^2 <= 1 + 1e-12, summed in the step anyway) with labels +-1, both comparator
 * losses take their closed form T/2 + x.theta_e/2 (every loss is linear on the ball and
 * theta_e = -S_T is in registers), so such waves read z once instead of twice; the rest
 * stream the second pass.  Equal to the sequential sums up to their rounding. */
#define OCX_ALG_CLOSED_COMPARATOR 2
/* OCX_ALG_TREE_SUMS (ocx_dev_ftrl_vs_exact_ex): butterfly sums even when the layout chains
 * (the tiling is the same): the fused kernel's four chained totals per step leave it
 * latency-bound where the plain FTRL kernel streams (32768 x 1e4 x 64, one pass: 43 ms
 * chained vs 28 ms butterfly); about 1e-16 relative instead of the sequential order.
 * ocx_ftrl_vs_exact_batch applies it for lanes_per_seq = OCX_LANES_BEST. */
#define OCX_ALG_TREE_SUMS 4
int ocx_dev_ftrl_vs_exact_ex(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                             double eta0, double* cum_ftrl, double* cum_exact, double* comp_exact,
                             double* comp_ftl, double* cmp_action, int32_t* regime, int norm,
                             int flags, void* stream);

/* FTRL-vs-exact-FTL regret curves: exact_ftl_driver.py:157-190 observed at K checkpoint
 * horizons in one pass.  Both loops of ocx_dev_ftrl_vs_exact_ex are online, so for checkpoints
 * 0 <= t_1 < ... < t_K <= T (strictly increasing; 0 and T allowed) column k of every output,
 *   cum_ftrl[b][k], cum_exact[b][k], comp_exact[b][k], comp_ftl[b][k], regime[b][k],
 *   cmp_action[b][k][:],
 * carries the bits ocx_dev_ftrl_vs_exact_ex gives on the batch truncated at t_k, with the same
 * layout (which does not depend on T), norm and flags; t_k = 0 gives zero losses.
 *
 * bytes of caller-owned device workspace for K checkpoints in layout L (with_comp_ftl: the call
 * will pass a comp_ftl output); 0 for K == 0 or an empty batch; negative ocx_status on error
 * (bad layout, K < 0, K > T + 1) */
int64_t ocx_ftrl_exact_curve_workspace_bytes(const ocx_layout* L, int64_t K, int with_comp_ftl);

/* device: checkpoints is a DEVICE int64 array [K], strictly increasing in [0, L->T] — a
 * precondition the call cannot see: an array that breaks it gives meaningless numbers, but the
 * kernels never leave the batch, the outputs and the workspace whatever it holds;
 * cum_ftrl / cum_exact / comp_exact: device [B][K] row-major, required; comp_ftl [B][K]
 * nullable; cmp_action [B][K][d] nullable; regime [B][K] int32, required; closed [B][K] int32
 * nullable (1 = both comparator losses in closed form);
 * norm, flags: as in ocx_dev_ftrl_vs_exact_ex (OCX_ALG_CLOSED_COMPARATOR / OCX_ALG_CLIPPED_ROWS,
 * OCX_ALG_TREE_SUMS).  The closed form is per (sequence, checkpoint): a pair the kernel cannot
 * certify — every pair with flags 0, every l1 / linf pair — gets the streamed pass over its
 * prefix, and a certified sequence keeps the closed form whatever shares its wave;
 * workspace: workspace_bytes >= ocx_ftrl_exact_curve_workspace_bytes(L, K, comp_ftl != NULL) of
 * device memory, 8-byte aligned, the call's own until the stream has passed it;
 * K == 0 and B == 0 launch nothing; T == 0 is valid;
 * asynchronous, no allocation, no sync: capture-safe like the other dev entry points.
 * Cost: one read of z when every pair takes the closed form; otherwise the prefixes of the
 * other pairs are read once more (at most sum_k t_k rows per sequence). */
int ocx_dev_ftrl_vs_exact_curve(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                                double eta0, const int64_t* checkpoints, int64_t K,
                                double* cum_ftrl, double* cum_exact, double* comp_exact,
                                double* comp_ftl, double* cmp_action, int32_t* regime,
                                int32_t* closed, int norm, int flags, void* workspace,
                                size_t workspace_bytes, void* stream);

/* host: numpy buffers in, [B][K] out (cmp_action [B][K][d]); checkpoints is a HOST array,
 * validated here (order, range, K >= 0) before any device is touched.  lanes_per_seq chooses the
 * closed form and the butterfly sums as ocx_ftrl_vs_exact_batch_ex does. */
int ocx_ftrl_vs_exact_curve_batch(const double* z, const double* y, int64_t B, int64_t T,
                                  int64_t d, double eta0, const int64_t* checkpoints, int64_t K,
                                  double* cum_ftrl, double* cum_exact, double* comp_exact,
                                  double* comp_ftl, double* cmp_action, int32_t* regime,
                                  int32_t* closed, int norm, int lanes_per_seq, int device);

/* FTRL-vs-exact-FTL regret grids: ocx_dev_ftrl_vs_exact_curve for M step sizes per read of z.
 * Of the two loops only FTRL depends on eta0, so one pass holds NE FTRL columns beside one
 * exact-FTL column.  For step sizes etas[0..M) (any reals, any order, duplicates allowed) and
 * checkpoints 0 <= t_1 < ... < t_K <= T,
 *   cum_ftrl[b][m][k], comp_ftl[b][m][k]                                        ([B][M][K])
 *   cum_exact[b][k], comp_exact[b][k], regime[b][k], closed[b][k], cmp_action[b][k][:]
 * carry the bits of ocx_dev_ftrl_vs_exact_curve(eta0 = etas[m]) at column k, with the same
 * layout, norm and flags — that is, of ocx_dev_ftrl_vs_exact_ex on the batch truncated at t_k.
 * The second line does not depend on eta0 and is written once.  A plain step-size sweep is the
 * grid with checkpoints = [T].
 *
 * step sizes one pass over z serves in layout L: 1, 2 or 4; negative ocx_status on a bad layout */
int ocx_ftrl_exact_grid_group(const ocx_layout* L);

/* bytes of caller-owned device workspace for M step sizes and K checkpoints in layout L, enough
 * for every `group` the layout offers; 0 for M == 0, K == 0 or an empty batch; negative
 * ocx_status on error (bad layout, M < 0, K < 0, K > T + 1) */
int64_t ocx_ftrl_exact_grid_workspace_bytes(const ocx_layout* L, int64_t M, int64_t K,
                                            int with_comp_ftl);

/* device: etas is a HOST array [M], read before the call returns; checkpoints a DEVICE int64
 * array [K] under ocx_dev_ftrl_vs_exact_curve's precondition and guarantee (whatever it holds,
 * the kernels never leave the batch, the outputs and the workspace);
 * cum_ftrl: device [B][M][K] row-major, required; comp_ftl [B][M][K] nullable; cum_exact /
 * comp_exact [B][K] and regime [B][K] int32 required; cmp_action [B][K][d] and closed [B][K]
 * int32 nullable; norm, flags: as in ocx_dev_ftrl_vs_exact_curve;
 * group: step sizes per pass, 0 = ocx_ftrl_exact_grid_group(L) (capped at what M needs), or 1,
 * 2, 4 where the layout has that instance (OCX_E_UNSUPPORTED otherwise).  With M above the
 * group the call runs ceil(M / group) passes; every pass re-runs the exact side, the first
 * writes its outputs.  The results do not depend on the group;
 * workspace: workspace_bytes >= ocx_ftrl_exact_grid_workspace_bytes(L, M, K, comp_ftl != NULL),
 * 8-byte aligned, the call's own until the stream has passed it;
 * M == 0, K == 0 and B == 0 launch nothing; asynchronous, no allocation, no sync. */
int ocx_dev_ftrl_vs_exact_curve_etas(const ocx_layout* L, const double* z_tiled,
                                     const double* y_tiled, const double* etas, int64_t M,
                                     const int64_t* checkpoints, int64_t K, double* cum_ftrl,
                                     double* cum_exact, double* comp_exact, double* comp_ftl,
                                     double* cmp_action, int32_t* regime, int32_t* closed,
                                     int norm, int flags, int group, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* host: numpy buffers in; cum_ftrl / comp_ftl [B][M][K], the others [B][K] (cmp_action
 * [B][K][d]) out; etas and checkpoints are HOST arrays, validated here (order, range, M >= 0,
 * K >= 0) before any device is touched.  lanes_per_seq chooses the closed form and the butterfly
 * sums as ocx_ftrl_vs_exact_curve_batch does. */
int ocx_ftrl_vs_exact_curve_etas_batch(const double* z, const double* y, int64_t B, int64_t T,
                                       int64_t d, const double* etas, int64_t M,
                                       const int64_t* checkpoints, int64_t K, double* cum_ftrl,
                                       double* cum_exact, double* comp_exact, double* comp_ftl,
                                       double* cmp_action, int32_t* regime, int32_t* closed,
                                       int norm, int lanes_per_seq, int device);

/* fast_algorithms.py:118-164 on device; thresh [B] device. */
int ocx_dev_simulate_smart(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                           const double* thresh, double eta0, double* regret,
                           int64_t* switch_step, void* stream);

/* ocx_dev_simulate_smart with options.  flags (bitwise or):
 *   OCX_SMART_CLOSED_PREFIX  O(T·d): the pre-switch prefix loss (:157-160) in closed form,
 *     (t+1)/2 − ½ s_t·S_t with S_t = Σ_{i<=t} y_i z_i, valid while every row is in the unit
 *     ball (||z_i||² <= 1 + 1e-12) and every label is ±1 (the kernel checks both).  It only
 *     decides the switch where ftl_loss − s_loss is farther from the threshold than a bound
 *     on the rounding that separates it from the reference's sequential sum; inside that
 *     band, or outside the regime, the step re-scans its prefix as the reference does.  The
 *     switch steps, hence the regrets, are the reference's.
 *   OCX_ALG_CLOSED_COMPARATOR  the final comparator loss of FTL(theta_ftl) as T/2 −
 *     ||theta_ftl|| where certified (as ocx_dev_simulate_alg_ex): one HBM pass in all, the
 *     regret then within the comparator sum's rounding of the reference's.
 * stats (nullable, device uint64 [2]): += steps that re-scanned, += sequences that took the
 * closed comparator. */
#define OCX_SMART_CLOSED_PREFIX 8
int ocx_dev_simulate_smart_ex(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                              const double* thresh, double eta0, double* regret,
                              int64_t* switch_step, int flags, unsigned long long* stats,
                              void* stream);

/* Threshold sweeps: SMART (fast_algorithms.py:118-164) for M switch thresholds in passes over
 * z that each serve a group of them.  The FTL leg, the prefix loss of the switch test and the
 * final comparator do not depend on the threshold and are formed once per pass; the switch
 * step, the FTRL state after it and total_loss are per column.  For every m,
 *   regret[b][m], switch_step[b][m]
 * are bit for bit what ocx_dev_simulate_smart_ex's lane-group kernel gives with
 * thresh[b] = thresh[b][m], the same layout and the same flags; they do not depend on the
 * group size in use.  thresh = +inf makes a column FTL's regret (the column never switches:
 * the same adds, the same comparator); sqrt(2T) and the empirical g(T) are the drivers' SMART
 * and EMP columns.  NaN and ±inf are legal thresholds (NaN and +inf never switch, -inf
 * switches at step 0), any order, duplicates allowed.
 *
 * thresholds one pass over z serves in layout L (1: once per threshold; negative ocx_status
 * on error).  Above 1 only where that group measured faster than M single-threshold passes
 * (DESIGN.md 3.11); never above the smallest group that holds M. */
int ocx_smart_thresholds_group(const ocx_layout* L, int64_t M);

/* device: thresh is a DEVICE array [B][M] row-major (per-sequence thresholds); regret [B][M]
 * device, switch_step [B][M] int64 device, nullable (-1 = never switched);
 * flags: those of ocx_dev_simulate_smart_ex (OCX_SMART_CLOSED_PREFIX,
 * OCX_ALG_CLOSED_COMPARATOR / OCX_ALG_CLIPPED_ROWS); unknown flags are rejected.  A step
 * whose closed-form prefix leaves some column undecided re-scans the prefix once for all of
 * them.  stats (nullable, device uint64 [2]), per launch (ceil(M / group) launches):
 * += (sequence, step) pairs that re-scanned, += sequences that took the closed comparator.
 * M == 0, B == 0 and T == 0 are valid (T == 0 gives zeros and -1);
 * asynchronous, no allocation, no sync: capture-safe like the other dev entry points.
 * With flags 0 and stats NULL in an exact layout (chain, or one lane per sequence) at d <= 64
 * and B <= 32768, this call and ocx_dev_simulate_smart_curve run the one-wave-per-sequence
 * kernel (up to eight columns per prefix re-scan) where it measured faster:
 * the same bits.  OCX_SMART_KERNEL=lanes in the environment holds them on the lane-group
 * kernel, as it does ocx_dev_simulate_smart. */
int ocx_dev_simulate_smart_thresholds(const ocx_layout* L, const double* z_tiled,
                                      const double* y_tiled, const double* thresh, int64_t M,
                                      double eta0, double* regret, int64_t* switch_step,
                                      int flags, unsigned long long* stats, void* stream);

/* host: numpy buffers in, [B][M] out; thresh is a HOST array [B][M]; switch_step nullable.
 * Bit-exact layouts (lanes_per_seq 1 / -k): flags 0, the reference's prefix re-scan (once per
 * step for the group's columns) and streamed comparator; other modes: both closed forms. */
int ocx_simulate_smart_thresholds_batch(const double* z, const double* y, int64_t B, int64_t T,
                                        int64_t d, const double* thresh, int64_t M, double eta0,
                                        double* regret, int64_t* switch_step, int lanes_per_seq,
                                        int device);

/* SMART regret curves: SMART (fast_algorithms.py:118-164) for K pairs (horizon t_k, threshold
 * thresh[b][k]) in passes over z that each serve a group of consecutive pairs.  The horizons
 * are NON-DECREASING in [0, T] (equal horizons are legal: SMART and EMP at the same t_k; with
 * every t_k = T this is the threshold sweep).  SMART's run on the first t rows is the first t
 * steps of its run on all of them — the FTL leg and the switch test's prefix loss depend on
 * neither the threshold nor the horizon, FTRL's step size on the global step — so for every k
 *   regret[b][k], switch_step[b][k]
 * are bit for bit what ocx_dev_simulate_smart_ex's lane-group kernel gives on
 * (z[b][:t_k], y[b][:t_k]) with thresh[b] = thresh[b][k], the same layout (it does not depend
 * on T) and the same flags.  switch_step lies in [0, t_k) or is -1; t_k = 0 gives 0.0 and -1.
 * A column freezes at its horizon: its loss as it stands, and as comparator FTL(theta_ftl
 * after t_k steps) over rows 0 .. t_k-1, streamed there in the reference's order or, with
 * OCX_ALG_CLOSED_COMPARATOR, t_k/2 - ||theta_ftl|| where the first t_k steps certify it.  The
 * certificate is per (sequence, column); a column's bits depend neither on the group size nor
 * on its neighbours.  A pass loops to its group's last horizon only, and a step re-scans only
 * while some column of the group is both unswitched and before its horizon.  NaN and ±inf
 * thresholds as in the threshold sweep; OCX_SMART_CLOSED_PREFIX and its guard band are
 * unchanged (they depend on t and d, never on T).
 *
 * pairs one pass over z serves in layout L (1: one pass per pair; negative ocx_status on
 * error).  Above 1 only where that group measured faster than K single-threshold calls on
 * truncated batches; never above the smallest group that holds K. */
int ocx_smart_curve_group(const ocx_layout* L, int64_t K);

/* device: horizons is a HOST array [K], read and validated (order, range) at call time: a bad
 * list returns OCX_E_INVALID and nothing is launched.  thresh is a DEVICE array [B][K]
 * row-major; regret [B][K] device, switch_step [B][K] int64 device, nullable.  flags: those of
 * ocx_dev_simulate_smart_ex; unknown flags are rejected.  stats (nullable, device uint64 [2]),
 * per launch (ceil(K / group) launches): += (sequence, step) pairs that re-scanned,
 * += (sequence, column) pairs that took the closed comparator.  K == 0, B == 0 and T == 0 are
 * valid; asynchronous, no allocation, no sync: capture-safe like the other dev entry points
 * (a captured graph keeps the horizons it was captured with). */
int ocx_dev_simulate_smart_curve(const ocx_layout* L, const double* z_tiled,
                                 const double* y_tiled, const int64_t* horizons,
                                 const double* thresh, int64_t K, double eta0, double* regret,
                                 int64_t* switch_step, int flags, unsigned long long* stats,
                                 void* stream);

/* host: numpy buffers in, [B][K] out; horizons HOST [K], thresh HOST [B][K]; switch_step
 * nullable.  Bit-exact layouts (lanes_per_seq 1 / -k): flags 0; other modes: both closed
 * forms, as ocx_simulate_smart_thresholds_batch. */
int ocx_simulate_smart_curve_batch(const double* z, const double* y, int64_t B, int64_t T,
                                   int64_t d, const int64_t* horizons, const double* thresh,
                                   int64_t K, double eta0, double* regret, int64_t* switch_step,
                                   int lanes_per_seq, int device);

/* SMART regret grids: SMART (fast_algorithms.py:118-164) for M thresholds, each observed at K
 * checkpoint horizons 0 <= t_1 < ... < t_K <= T, in passes over z that each serve a group of
 * thresholds and run once, to t_K.  The surface R(threshold, T) as a pair list
 * (ocx_dev_simulate_smart_curve over M*K pairs) computes every trajectory K times: a
 * threshold's column at t_k and at t_{k+1} are the same run.  Here the FTL leg, the prefix loss
 * of the switch test and the comparator of a checkpoint are formed once per pass; no column
 * freezes.  Outputs are [B][M][K] row-major, and for every (m, k)
 *   regret[b][m][k], switch_step[b][m][k]
 * are bit for bit what ocx_dev_simulate_smart_ex's lane-group kernel gives on
 * (z[b][:t_k], y[b][:t_k]) with thresh[b] = thresh[b][m], the same layout and the same flags.
 * So [:, m, :] is ocx_dev_simulate_smart_curve on (t_k, thresh[.][m]) for every k, and with
 * t_K = T, [:, :, K-1] is ocx_dev_simulate_smart_thresholds.  switch_step[b][m][k] is the full
 * run's step s where 0 <= s < t_k, else -1; t_k = 0 gives 0.0 and -1; thresh = +inf is FTL's
 * regret at every horizon.  The result depends neither on the group size nor on a column's
 * neighbours.  NaN and +-inf thresholds as in the threshold sweep, any order, duplicates
 * allowed; OCX_SMART_CLOSED_PREFIX and its guard band are unchanged.  The closed comparator
 * (OCX_ALG_CLOSED_COMPARATOR) is certified per (sequence, checkpoint) by that prefix's steps;
 * an uncertified pair streams rows 0 .. t_k-1 in place, once for all columns of the pass.  A
 * pass never looks past t_K and needs no workspace.
 *
 * thresholds one pass over z serves in layout L (1: one pass per threshold; negative
 * ocx_status on error).  Never above the smallest group that holds M; 1 for M <= 1
 * (DESIGN.md 3.17). */
int ocx_smart_grid_group(const ocx_layout* L, int64_t M);

/* device: thresh is a DEVICE array [B][M] row-major; checkpoints is a DEVICE int64 array [K],
 * strictly increasing in [0, T].  It cannot be validated without a synchronisation: a bad
 * list is the caller's error and gives meaningless numbers, but the kernels never leave the
 * batch or the outputs, and terminate (a checkpoint is clamped to [0, T]; a segment that
 * would go backwards is empty).  regret [B][M][K] device, switch_step [B][M][K] int64 device,
 * nullable.  flags: those of ocx_dev_simulate_smart_ex; unknown flags and NULL arrays are
 * OCX_E_INVALID before anything is launched.  stats (nullable, device uint64 [2]), per launch
 * (ceil(M / group) launches): += (sequence, step) pairs that re-scanned (a step re-scans only
 * while some column of the launch is unswitched and the step is before t_K), += (sequence,
 * column, checkpoint) triples that took the closed comparator.  M == 0, K == 0, B == 0 and
 * T == 0 are valid; asynchronous, no allocation, no sync: capture-safe like the other dev
 * entry points (a replayed graph reads the checkpoints the device array then holds).  With
 * flags 0 and stats NULL in an exact layout at d <= 64 and B <= 32768 the
 * one-wave-per-sequence form runs (up to eight columns per prefix re-scan and per comparator
 * scan; at every M, where the sweeps keep M <= 4 columns on the lane-group kernel above d = 32:
 * DESIGN.md 3.17): the same bits.  OCX_SMART_KERNEL=lanes|wave is honoured as there. */
int ocx_dev_simulate_smart_grid(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                                const double* thresh, int64_t M, const int64_t* checkpoints,
                                int64_t K, double eta0, double* regret, int64_t* switch_step,
                                int flags, unsigned long long* stats, void* stream);

/* host: numpy buffers in, [B][M][K] out; thresh HOST [B][M], checkpoints HOST [K], whose order
 * and range, the counts and the NULLs are checked before a device is touched; switch_step
 * nullable.  Bit-exact layouts (lanes_per_seq 1 / -k): flags 0; other modes: both closed
 * forms, as ocx_simulate_smart_thresholds_batch. */
int ocx_simulate_smart_grid_batch(const double* z, const double* y, int64_t B, int64_t T,
                                  int64_t d, const double* thresh, int64_t M,
                                  const int64_t* checkpoints, int64_t K, double eta0,
                                  double* regret, int64_t* switch_step, int lanes_per_seq,
                                  int device);

/* exact_ftl.py:306-333 on device; a_tiled is the actions [B][T+1][d] tiled with a
 * layout of T+1 steps (z/y use L, actions use La with La->T == L->T + 1). */
int ocx_dev_replay(const ocx_layout* L, const ocx_layout* La, const double* z_tiled,
                   const double* y_tiled, const double* a_tiled, double* cum_loss,
                   double* comp_loss, void* stream);

/* ocx_exact_ball_solve on device: z [B][T][d], y [B][T] row-major (device), outputs as
 * there (device); runs on `stream`, does not synchronise. */
int ocx_dev_exact_ball_solve(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                             int norm, int all_prefixes, double* actions, double* obj, double* gap,
                             double* step_loss, int32_t* info, void* stream);
/* The same on a resident batch in the tiled layout L. */
int ocx_dev_exact_ball_solve_tiled(const ocx_layout* L, const double* z_tiled,
                                   const double* y_tiled, int norm, int all_prefixes,
                                   double* actions, double* obj, double* gap, double* step_loss,
                                   int32_t* info, void* stream);

/* Max over runs of regrets[B] (device) into *gmax (device), starting from 0.0
 * as fast_algorithms.py:228,242-243 does. */
int ocx_dev_max_regret(const double* regrets, int64_t B, double* gmax, void* stream);

/* fast_algorithms.py:230-247's inner loop over resident batches: for k < nbatch, the runs
 * run0 + k*B .. run0 + (k+1)*B - 1 are generated on device into z_tiled / y_tiled
 * (ocx_dev_gen_gT) and simulated by FTRL (alg_flag 0, eta0; the certified closed-form
 * comparator unless OCX_GENSIM_TWO_PASS, as ocx_gT_regrets does).  regret [B] (device,
 * required: every batch's regrets pass through it) holds the last batch's regrets; gmax (device double, nullable) receives
 * max(0, max over every batch's regrets), bit-identical to the host loop.  Queued on
 * `stream`; complete when the stream reaches this point.
 *   Pipelined (the default where supported: d = 64 with the 8 x 8 or 16 x 4 butterfly
 * layout, d = 16 / 32 with 8 lanes of 2 / 4 coordinates — the g(T) layouts — and a batch of
 * at least four generator rounds unless sub_seqs > 0 asks for it): the batch is cut into
 * sub-batches of sequences (sub_seqs, <= 0: generator rounds making about 64 000 normals per
 * stream, one to four) and sub-batch i+1 is generated while the FTRL kernel reads
 * sub-batch i, the sub-batches alternating over two library streams per side (forked from
 * and joined to `stream` by events), the generator at four 96-VGPR waves per SIMD and the
 * FTRL kernel in a 128-VGPR form so both stay resident (csrc/ocx_pipeline.hip); consecutive
 * batches overlap the same way.  On a stream under graph capture the sequential loop runs
 * instead.  Same kernels and arithmetic as the sequential path: the regrets are
 * bit-identical to it.
 *   OCX_GENSIM_SEQUENTIAL: generate, then simulate, batch by batch on `stream` (any layout).
 *   OCX_GENSIM_TWO_PASS: the reference's streamed comparator pass instead of the certified
 *     closed form (what the bit-exact layouts ask for; the regrets are then bit-identical to
 *     fast_algorithms.py in those layouts). */
#define OCX_GENSIM_SEQUENTIAL 1u
#define OCX_GENSIM_TWO_PASS 2u
int ocx_dev_gen_simulate(const ocx_layout* L, uint64_t base_seed, int64_t run0, int64_t nbatch,
                         double* z_tiled, double* y_tiled, double eta0, double* regret,
                         double* gmax, uint32_t flags, int64_t sub_seqs, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* OCX_H_ */
