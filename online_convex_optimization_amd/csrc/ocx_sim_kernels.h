// ocx_sim_kernels.h — host-side launchers for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocx.h"

bool ocx_supported_C(int C);
// algo: 0 FTRL, 1 FTL, 2 exact FTL (l2 ball, linear regime; see ocx_sim.hip).
// onepass: rows are known to satisfy ||z_t|| <= 1 (g(T) sampler): the comparator loss of
// FTL(theta_T) in closed form where the kernel can certify it (ocx_alg_kernel)
hipError_t ocx_launch_alg(const ocx_layout* L, const double* zt, const double* yt, int algo,
                          double eta0, const double* cmp, double* reg, double* cum, double* comp,
                          double* xl, hipStream_t st, double* cmp_out = nullptr,
                          int* regime = nullptr, int onepass = 0, int norm = 0,
                          const uint64_t* yb = nullptr);
// The label-bit tile (include/ocx.h, ocx_label_bits_words): yb, where a launcher takes it, is
// nullable and must describe the same labels as yt, every label of a real sequence ±1.  The
// instances of the pipelined step that read it: ocx_alg_pipe.hip.
int64_t ocx_label_bits_words_of(const ocx_layout* L);
// the tile of a row-major y [B][T]; *flag (device) = 1 if a real label is not exactly ±1
hipError_t ocx_launch_pack_ybits(const ocx_layout* L, const double* y, uint64_t* yb, int* flag,
                                 hipStream_t st);
// FTRL / FTL for butterfly layouts (chain = 0, P >= 2, C <= 32) with the step's dependency
// chain cut short (ocx_alg_pipe.hip); no comparator input, x_last or comparator output
bool ocx_pipe_supported(const ocx_layout* L);
hipError_t ocx_launch_alg_pipe(const ocx_layout* L, const double* zt, const double* yt, int ftl,
                               double eta0, double* reg, double* cum, double* comp,
                               int* closed_out, int onepass, hipStream_t st,
                               const uint64_t* yb = nullptr);
// its persistent instance (a batch of more groups than are resident at once: each wave loops
// over its share) with `nwaves` waves, whatever the batch's size; the layouts that have one
bool ocx_pipe_persistent_supported(const ocx_layout* L);
hipError_t ocx_launch_alg_pipe_persistent(const ocx_layout* L, const double* zt, const double* yt,
                                          int ftl, double eta0, double* reg, double* cum,
                                          double* comp, int* closed_out, int onepass,
                                          int64_t nwaves, hipStream_t st,
                                          const uint64_t* yb = nullptr);
// Regret curves (ocx_alg_curve.hip): FTRL / FTL observed at the K checkpoints ck (device,
// strictly increasing in [0, T]) in one pass; outputs [B][K] (each nullable).  The curve form
// of the pipelined kernel where ocx_pipe_supported(L), of the plain kernel otherwise; then
// the streamed comparator of the pairs the closed form (onepass) did not take, from ws
// (ocx_curve_ws_bytes(L, K) bytes of device memory).
int64_t ocx_curve_ws_bytes(const ocx_layout* L, int64_t K);
hipError_t ocx_launch_alg_curve(const ocx_layout* L, const double* zt, const double* yt, int ftl,
                                double eta0, const int64_t* ck, int64_t K, double* reg,
                                double* cum, double* comp, int* closed_out, int onepass,
                                void* ws, hipStream_t st);
// Anytime regret (ocx_alg_anytime.hip): the running max of the closed-form regret over every
// prefix t = 1 … T, and the smallest t attaining it, emitted at the K checkpoints ck (device,
// strictly increasing in [1, T]): sup / argsup [B][K]; open_from [B], the first t the kernel
// could not certify (T + 1: none; nothing after it enters the max); trace, in y_tiled's layout,
// the regret of every step (NaN where not certified).  Each output nullable.  One pass over z,
// no workspace, the curve's dispatch (the pipelined loop where ocx_pipe_supported(L)).
hipError_t ocx_launch_alg_anytime(const ocx_layout* L, const double* zt, const double* yt, int ftl,
                                  double eta0, const int64_t* ck, int64_t K, double* sup,
                                  int64_t* argsup, int64_t* open_from, double* trace, int onepass,
                                  hipStream_t st);
// Step-size sweeps (ocx_alg_etas.hip): FTRL for the M step sizes etas (HOST, read at call
// time) in passes of at most `group` (1, 2 or 4; ocx_etas_instance) columns; outputs [B][M]
// (each nullable).  The multi-η form of the pipelined kernel where ocx_pipe_supported(L), of
// the plain kernel otherwise.  ocx_etas_best_group: the group the measurements chose.
bool ocx_etas_instance(const ocx_layout* L, int group);
int ocx_etas_best_group(const ocx_layout* L);
hipError_t ocx_launch_alg_etas(const ocx_layout* L, const double* zt, const double* yt,
                               const double* etas, int64_t M, double* reg, double* cum,
                               double* comp, int* closed_out, int onepass, int group,
                               hipStream_t st);
// Regret grids (ocx_alg_curve_etas.hip): FTRL for the M step sizes etas (HOST, read at call
// time), each observed at the K checkpoints ck (device, strictly increasing in [0, T]), in
// passes of at most `group` (1, 2 or 4; ocx_grid_instance) step sizes; outputs [B][M][K] (each
// nullable).  Each pass is followed by the streamed comparator of the triples the closed form
// (onepass) did not take, from ws (ocx_grid_ws_bytes(L, K, min(group, M)) bytes of device
// memory, reused by the next pass).  ocx_grid_best_group: the group the measurements chose.
bool ocx_grid_instance(const ocx_layout* L, int group);
int ocx_grid_best_group(const ocx_layout* L);
int64_t ocx_grid_ws_bytes(const ocx_layout* L, int64_t K, int64_t ne);
hipError_t ocx_launch_alg_grid(const ocx_layout* L, const double* zt, const double* yt,
                               const double* etas, int64_t M, const int64_t* ck, int64_t K,
                               double* reg, double* cum, double* comp, int* closed_out,
                               int onepass, int group, void* ws, hipStream_t st);
// gmax[n] = max(start, max_b r[b][n]) over r [B][N]; start +0.0, or gmax[n] with accumulate
hipError_t ocx_launch_max_cols(const double* r, int64_t B, int64_t N, double* gmax,
                               int accumulate, hipStream_t st);
// the lean form over wave-groups [g0, g0 + gn) (<= 128 VGPRs; FTRL, 8 x 8 and 16 x 4 layouts),
// the FTRL side of the overlapped pipeline (ocx_pipeline.hip)
bool ocx_pipe_lean_supported(const ocx_layout* L);
// gmax (nullable, device): g(T)'s bit pattern, max-folded in the kernel (ocx_max_fold's rule)
hipError_t ocx_launch_alg_pipe_lean(const ocx_layout* L, const double* zt, const double* yt,
                                    double eta0, double* reg, int onepass, int64_t g0,
                                    int64_t gn, unsigned long long* gmax, hipStream_t st);
// FTRL over steps [t0, t0 + tn) of every sequence (t0 a multiple of 64), the step's state
// carried in `state` (ocx_pipe_state_doubles(L) doubles) from the chunk before; the chunk that
// ends at T writes the regrets (closed-form comparator only: onepass; a sequence it cannot
// certify gets NaN and sets *bad).  Bit-identical to one whole-horizon launch.
int64_t ocx_pipe_state_doubles(const ocx_layout* L);
hipError_t ocx_launch_alg_pipe_chunk(const ocx_layout* L, const double* zt, const double* yt,
                                     double eta0, double* reg, int onepass, int64_t t0,
                                     int64_t tn, double* state, int* bad,
                                     unsigned long long* gmax, hipStream_t st);
// g(T) sampler over sequences [b_off, b_off + nseq) of a d = 64 layout, at most wps waves per
// SIMD (four-wave blocks; ocx_gen_wave.hip)
// (wps >= 4: the 96-VGPR form, which spills a little; below: the 128-VGPR form)
hipError_t ocx_launch_gen_gT_range(const ocx_layout* L, uint64_t base_seed, int64_t run0,
                                   int64_t b_off, int64_t nseq, int wps, double* zt, double* ytl,
                                   hipStream_t st, uint64_t* ybits = nullptr);
// generation overlapped with FTRL (ocx_pipeline.hip): nbatch batches of L->B runs from run0,
// regret = the last batch's; gmax (nullable, device) max-folds g(T) over every batch
bool ocx_pipeline_supported(const ocx_layout* L);
bool ocx_pipeline_worth(const ocx_layout* L, int wps);
// the multi-stream paths may fork from st (not under graph capture on HIP runtimes < 7.2)
bool ocx_stream_fork_ok(hipStream_t st);
hipError_t ocx_launch_gen_gT_range_lr(const ocx_layout* L, uint64_t base_seed, int64_t run0,
                                      int64_t b_off, int64_t nseq, double* zt, double* ytl,
                                      hipStream_t st, uint64_t* ybits = nullptr);
// generation alone in rounds over two streams (ocx_pipeline.hip)
hipError_t ocx_run_gen_rounds(const ocx_layout* L, uint64_t base_seed, int64_t run0, double* zt,
                              double* yt, hipStream_t st, uint64_t* ybits = nullptr);
hipError_t ocx_run_gen_sim_pipelined(const ocx_layout* L, uint64_t base_seed, int64_t run0,
                                     int64_t nbatch, double* zt, double* yt, double eta0,
                                     double* regret, int onepass, unsigned long long* gmax,
                                     int wps, int64_t sub_seqs, hipStream_t st);
// generation of batch k+1 trailing the chunked FTRL pass over batch k in one z buffer
// (ocx_pipeline.hip: the capacity-limited batches); see there for the buffers
bool ocx_pipe_lean_launchable(const ocx_layout* L);  // ocx_launch_alg_pipe_lean's layouts
bool ocx_trailing_supported(const ocx_layout* L);
// the largest batch whose generator waves all fit beside the FTRL chunks' waves
int64_t ocx_trailing_max_batch(const ocx_layout* L);
int64_t ocx_trailing_batches_run();  // batches through ocx_run_gen_sim_trailing so far
hipError_t ocx_run_gen_sim_trailing(const ocx_layout* L, uint64_t base_seed, int64_t run0,
                                    int64_t nbatch, double* zt, double* yt0, double* yt1,
                                    uint64_t* gst, double* fst, int* bad, double eta0,
                                    double* regret, int64_t last_B, unsigned long long* gmax,
                                    int nchunks, hipStream_t st);
// rows [t_off, t_off + nrows) of L's full-horizon tile, streams fresh (st_in null) or resumed
// from st_in, saved to st_out (nullable, not st_in); labels: then the T labels (ocx_gen_wave.hip)
hipError_t ocx_launch_gen_gT_rows(const ocx_layout* L, uint64_t base_seed, int64_t run0,
                                  int64_t t_off, int64_t nrows, const uint64_t* st_in,
                                  uint64_t* st_out, int labels, double* zt, double* ytl,
                                  hipStream_t st);
// the general exact comparator for 10 < d <= 64 (ocx_exact_wide.hip): row-major z/y
// (tiled = 0) or a tiled layout's (P, C, S, G)
hipError_t ocx_launch_exact_wide(const double* z, const double* y, int64_t B, int64_t T,
                                 int64_t d, int tiled, int P, int C, int S, int64_t G, int norm,
                                 int all_prefixes, double* actions, double* obj, double* gap,
                                 double* step_loss, int32_t* info, hipStream_t st);
// the general solvers' certificate polish (ocx_exact_wide.hip): the actions purified onto
// their active face and a dual rebuilt from the KKT system there; where that certifies a
// smaller gap, actions, obj, gap and step_loss are replaced.  d <= 64
hipError_t ocx_launch_exact_polish(const double* z, const double* y, int64_t B, int64_t T,
                                   int64_t d, int tiled, int P, int C, int S, int64_t G, int norm,
                                   int all_prefixes, double* actions, double* obj, double* gap,
                                   double* step_loss, hipStream_t st);
// the general exact comparator for 64 < d <= 256 (ocx_exact_big.hip): the solve and its
// certificate polish, the system in a per-block HBM scratch matrix
hipError_t ocx_launch_exact_big(const double* z, const double* y, int64_t B, int64_t T, int64_t d,
                                int tiled, int P, int C, int S, int64_t G, int norm,
                                int all_prefixes, double* actions, double* obj, double* gap,
                                double* step_loss, int32_t* info, hipStream_t st);
hipError_t ocx_launch_smart(const ocx_layout* L, const double* zt, const double* yt,
                            const double* th, double eta0, double* reg, int64_t* sw,
                            hipStream_t st);
// SMART in lane-group form (ocx_smart_thresholds.hip, one kernel with 1, 2 or 4 threshold
// columns): closed_prefix decides the switch from the closed-form prefix loss outside a
// rounding guard band (re-scan inside it: the reference's decisions), O(T·d); closed_comp takes
// the final comparator loss in closed form where certified.
// stats (nullable, device [2]): += re-scanned steps, += sequences with the closed comparator
// One threshold per sequence, th / reg / sw [B]: one launch of the one-column instance.
hipError_t ocx_launch_smart_closed(const ocx_layout* L, const double* zt, const double* yt,
                                   const double* th, double eta0, double* reg, int64_t* sw,
                                   int closed_prefix, int closed_comp, unsigned long long* stats,
                                   hipStream_t st);
// Threshold sweeps: the M thresholds th [B][M] (device) in passes of at most `group` (1, 2 or
// 4; ocx_thresholds_instance) columns, each column the bits of ocx_launch_smart_closed with
// that threshold; reg / sw [B][M] (sw nullable); stats per launch.  ocx_thresholds_best_group: the
// group the measurements chose.
bool ocx_thresholds_instance(const ocx_layout* L, int group);
int ocx_thresholds_best_group(const ocx_layout* L);
hipError_t ocx_launch_smart_thresholds(const ocx_layout* L, const double* zt, const double* yt,
                                       const double* th, int64_t M, double eta0, double* reg,
                                       int64_t* sw, int closed_prefix, int closed_comp,
                                       unsigned long long* stats, int group, hipStream_t st);
// SMART regret curves (ocx_smart_curve.hip): the K pairs (horizon hz[k], HOST, read at call
// time, non-decreasing in [0, T]; threshold th[b][k], device) in passes of at most `group`
// (1, 2 or 4; ocx_smart_curve_instance) consecutive pairs, each looping to its last horizon;
// column k the bits of ocx_launch_smart_closed on the rows truncated at hz[k]; reg / sw
// [B][K] (sw nullable); stats per launch: += re-scanned (sequence, step) pairs, += (sequence,
// column) pairs with the closed comparator.  ocx_smart_curve_best_group: the group the
// measurements chose.
bool ocx_smart_curve_instance(const ocx_layout* L, int group);
int ocx_smart_curve_best_group(const ocx_layout* L);
hipError_t ocx_launch_smart_curve(const ocx_layout* L, const double* zt, const double* yt,
                                  const int64_t* hz, const double* th, int64_t K, double eta0,
                                  double* reg, int64_t* sw, int closed_prefix, int closed_comp,
                                  unsigned long long* stats, int group, hipStream_t st);
// SMART with one wavefront per sequence (ocx_smart_wave.hip), d <= 64.  ocx_smart_wave_sizes:
// the sizes at which ocx_launch_smart takes it, and the sweeps' dispatch its column form.
bool ocx_smart_wave_sizes(const ocx_layout* L);
hipError_t ocx_launch_smart_wave(const ocx_layout* L, const double* zt, const double* yt,
                                 const double* th, double eta0, double* reg, int64_t* sw,
                                 hipStream_t st);
// its NT-column form (ocx_smart_wave_cols.hip), re-scan mode only, d <= 64 (else
// hipErrorNotSupported): the M pairs (horizon hz[m], HOST, read at call time, non-decreasing in
// [0, T]; NULL: every horizon T, the threshold sweep; threshold th[b][m], device) in launches
// of at most `group` (1, 2, 4 or 8) consecutive columns, one prefix re-scan per step for all of
// a launch's columns; column m the bits of ocx_launch_smart_wave on the rows truncated at
// hz[m] — the reference's summation order in any layout; reg / sw [B][M] (sw nullable);
// stats[0] (nullable) += (sequence, step) pairs whose switch test ran, per launch.  Allocates
// nothing and never synchronises.  ocx_smart_wave_cols_group: the group the measurements chose;
// ocx_smart_wave_cols_worth: whether they found this form faster than the lane-group sweep and
// than M single calls for M columns of this layout (the sweeps' dispatch asks).
bool ocx_smart_wave_cols_instance(int group);
int ocx_smart_wave_cols_group(const ocx_layout* L, int64_t M);
bool ocx_smart_wave_cols_worth(const ocx_layout* L, int64_t M);
hipError_t ocx_launch_smart_wave_cols(const ocx_layout* L, const double* zt, const double* yt,
                                      const int64_t* hz, const double* th, int64_t M, double eta0,
                                      double* reg, int64_t* sw, unsigned long long* stats,
                                      int group, hipStream_t st);
hipError_t ocx_launch_replay(const ocx_layout* L, const double* zt, const double* yt,
                             const double* at, double* cum, double* comp, hipStream_t st);
// exact FTL prefix actions [B][T+1][d] (closed form, l2 ball; ocx_sim.hip)
hipError_t ocx_launch_prefix_actions(const ocx_layout* L, const double* zt, const double* yt,
                                     double* actions, int* regime, hipStream_t st, int norm = 0);
hipError_t ocx_launch_pack(const ocx_layout* L, const double* z, const double* y, double* zt,
                           double* ytl, hipStream_t st);
hipError_t ocx_launch_max(const double* r, int64_t B, double* out, hipStream_t st);
int64_t ocx_gen_resident_waves(int64_t d, int dev);  // streams the generator runs in one round
// FTRL over wave-groups [g0, g0 + gn) of the 8 x 2 tree layout (the small-d pipeline's FTRL side
// at d = 16), g(T) folded into gmax (nullable)
hipError_t ocx_launch_alg_range(const ocx_layout* L, const double* zt, const double* yt,
                                double eta0, double* reg, int onepass, int64_t g0, int64_t gn,
                                unsigned long long* gmax, hipStream_t st);
// ybits (nullable): the label-bit tile, filled beside ytl
hipError_t ocx_launch_gen_gT(const ocx_layout* L, uint64_t base_seed, int64_t run0, double* zt,
                             double* ytl, hipStream_t st, uint64_t* ybits = nullptr);
// the g(T) sampler's normals unclipped (the float32 twin clips them itself)
hipError_t ocx_launch_gen_gT_raw(const ocx_layout* L, uint64_t base_seed, int64_t run0, double* zt,
                                 double* ytl, hipStream_t st);
hipError_t ocx_launch_gen_family(const ocx_layout* L, int family, const uint64_t* run_seeds,
                                 const uint64_t* stream_ids, double p, int64_t block_len,
                                 double* zt, double* ytl, hipStream_t st);
hipError_t ocx_launch_gen_seek(uint64_t base_seed, int64_t T_seed, int64_t run0, int64_t B,
                               int64_t d, uint64_t* st_out, uint64_t* lab_out, hipStream_t st);
hipError_t ocx_launch_gen_gT_chunk(const ocx_layout* L, int64_t T_seed, const uint64_t* st_in,
                                   uint64_t* st_out, const uint64_t* lab_in, uint64_t* lab_out,
                                   double* zt, double* ytl, hipStream_t st);
// mode 0 pass A, 1 pass B, 2 closed-form comparator (ocx_stream.hip); unclean [B + 1]
hipError_t ocx_launch_alg_chunk(const ocx_layout* L, const double* zt, const double* yt,
                                int64_t t0, int alg_flag, double eta0, int mode, double* theta,
                                double* cum, double* comp, double* regret, hipStream_t st,
                                double* unclean = nullptr);
// FTRL and exact FTL in one pass (ocx_ftrl_exact.hip)
hipError_t ocx_launch_ftrl_exact(const ocx_layout* L, const double* zt, const double* yt,
                                 double eta0, double* cum_r, double* cum_e, double* comp_e,
                                 double* comp_f, double* cmp_out, int* regime, hipStream_t st,
                                 int onepass = 0, int norm = 0);
// Its curve form (ocx_ftrl_exact_curve.hip): both loops observed at the K checkpoints ck (device,
// strictly increasing in [0, T]) in one pass; cum_r / cum_e / comp_e / regime [B][K], comp_f and
// closed_out [B][K] nullable, cmp_out [B][K][d] nullable.  Then the streamed comparator of the
// pairs the closed form did not take, from ws (ocx_ftrl_exact_curve_ws_bytes bytes of device
// memory; with_comp_f: comp_f != nullptr).
int64_t ocx_ftrl_exact_curve_ws_bytes(const ocx_layout* L, int64_t K, int with_comp_f);
hipError_t ocx_launch_ftrl_exact_curve(const ocx_layout* L, const double* zt, const double* yt,
                                       double eta0, const int64_t* ck, int64_t K, double* cum_r,
                                       double* cum_e, double* comp_e, double* comp_f,
                                       double* cmp_out, int* regime, int* closed_out, int onepass,
                                       int norm, void* ws, hipStream_t st);
// Its step-size form (ocx_ftrl_exact_grid.hip): FTRL for the M step sizes etas (HOST, read at
// call time) beside one exact-FTL column, observed at the K checkpoints, in passes of `group`
// (1, 2, 4; ocx_ftrl_exact_grid_instance) step sizes.  cum_r / comp_f [B][M][K]; the others as in
// the curve form, written by the first pass.  ws: ocx_ftrl_exact_grid_ws_bytes(L, K, ne,
// with_comp_f) bytes for passes of up to ne columns.
bool ocx_ftrl_exact_grid_instance(const ocx_layout* L, int group);
int ocx_ftrl_exact_grid_best_group(const ocx_layout* L);
int64_t ocx_ftrl_exact_grid_ws_bytes(const ocx_layout* L, int64_t K, int64_t ne, int with_comp_f);
hipError_t ocx_launch_ftrl_exact_grid(const ocx_layout* L, const double* zt, const double* yt,
                                      const double* etas, int64_t M, const int64_t* ck, int64_t K,
                                      double* cum_r, double* cum_e, double* comp_e, double* comp_f,
                                      double* cmp_out, int* regime, int* closed_out, int onepass,
                                      int norm, int group, void* ws, hipStream_t st);
// float32 twin (algorithms.py, ocx_twin32.hip): P = 1 layouts, d <= 32
// algo 0 FTRL, 1 FTL, 2 SMART (thresh[B]); clip: rows are raw g(T) normals to round to
// float and clip in float32 (algorithms.py:157-160)
hipError_t ocx_launch_twin32(const ocx_layout* L, const double* zt, const double* yt, int algo,
                             double eta0, const double* thresh, int clip, float* result,
                             double* cum, float* comp, int64_t* sw, hipStream_t st);
hipError_t ocx_launch_pack32(const ocx_layout* L, const float* z, const float* y, double* zt,
                             double* ytl, hipStream_t st);
// Its column form (ocx_twin32_cols.hip): K columns (hz[k], algos[k], thresh[b][k]), hz / algos
// HOST arrays the caller has validated (hz non-decreasing in [0, T], algos in 0..2), in launches
// of `group` (1, 2, 4, 8; <= ocx_twin32_cols_max_group) consecutive columns; one wavefront per
// sequence, rows [0, group's last horizon) staged in LDS.  result [B][K]; cum / comp / sw
// [B][K] nullable.  hipErrorNotSupported, before any launch, when hz[K - 1] exceeds
// ocx_twin32_cols_max_horizon(L).
int ocx_twin32_cols_max_group(const ocx_layout* L);
int64_t ocx_twin32_cols_max_horizon(const ocx_layout* L);
hipError_t ocx_launch_twin32_cols(const ocx_layout* L, const double* zt, const double* yt,
                                  int64_t K, const int64_t* hz, const int32_t* algos, double eta0,
                                  const double* thresh, float* result, double* cum, float* comp,
                                  int64_t* sw, int group, hipStream_t st);
// exact_ftl.py:224-227 `_comparator_loss` in OpenBLAS / NumPy order (ocx_comp_blas.hip):
// z [B][T][d] and y [B][T] row-major, x [B][d]; absr scratch [B][T]
hipError_t ocx_launch_comp_blas(const double* z, const double* y, const double* x, int64_t B,
                                int64_t T, int64_t d, double* absr, double* comp, hipStream_t st);
// The general exact-FTL comparator (ocx_exact_ball.hip): z [B][T][d], y [B][T] row-major;
// problems (b, n) for n = T … T-NP+1 (NP = all_prefixes ? T+1 : 1); actions [B][NP][d],
// obj / gap [B][NP] and info [B][NP] (Newton steps, negative at the iteration cap).
// d in 1..10.
// step_loss [B][NP] (nullable): ½|z_n·x_n − y_n|, the loss FTL pays at step n with the
// prefix-n action (0 for n = T).  The tiled form reads z / y in L's layout.
hipError_t ocx_launch_exact_ball(const double* z, const double* y, int64_t B, int64_t T,
                                 int64_t d, int norm, int all_prefixes, double* actions,
                                 double* obj, double* gap, double* step_loss, int32_t* info,
                                 hipStream_t st);
hipError_t ocx_launch_exact_ball_tiled(const ocx_layout* L, const double* zt, const double* yt,
                                       int norm, int all_prefixes, double* actions, double* obj,
                                       double* gap, double* step_loss, int32_t* info,
                                       hipStream_t st);
