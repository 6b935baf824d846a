/*
 * ocx_testing.h — test-only entry points of libocx.so (not part of the drop-in boundary).
 *
 * They exercise paths that correct inputs never reach, so the test suite can check them
 * without a process-wide switch in the product entry points.
 */
#ifndef OCX_TESTING_H_
#define OCX_TESTING_H_

#include <stdint.h>

#include "ocx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ocx_gT_regrets, but on the streamed (T-chunked) path every run r0 + b of a streamed
 * batch with b % unclean_every == 0 is treated as if it had failed the closed-form
 * comparator's check, so it takes the regenerated second pass (bit-identical to the
 * two-pass kernel); on the trailing path (resident batches of generation behind a chunked
 * FTRL pass) every batch k with k % unclean_every == 0 runs again whole, as a batch with a
 * NaN-flagged sequence does.  unclean_every >= 1. */
int ocx_test_gT_regrets_unclean(uint64_t base_seed, int64_t T, int64_t run0, int64_t R,
                                int64_t d, double eta0, double* regrets, int lanes_per_seq,
                                int device, int64_t unclean_every);

/* The trailing pipeline's FTRL side on a resident batch: the pipelined FTRL kernel run in
 * launches of chunk_steps steps (a multiple of 64), its state carried through device memory
 * between them, closed-form comparator.  regret [B] (device): bit-identical to one launch
 * for every sequence the closed form certifies; NaN for the others, and *bad (device int,
 * zeroed by the caller) set to 1.  Synchronises `stream`.  Butterfly layouts the pipelined
 * kernel takes (P in {8, 16, 32}, C in {4, 8, 16, 32}, and P = 64 with C = 16); any other
 * layout is OCX_E_UNSUPPORTED. */
int ocx_test_alg_pipe_chunked(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                              double eta0, int64_t chunk_steps, double* regret, int* bad,
                              void* stream);

/* The sub-batch pipeline's FTRL launch on a resident batch: FTRL over wave-groups
 * [g0, g0 + gn) of the layout (group g holds sequences g*S .. g*S + S - 1), dispatched as the
 * pipeline dispatches it — the pipelined kernel's lean whole-run form where the pipelined
 * kernel takes the layout (8 x 8, 16 x 4, 8 x 4), the plain kernel over a group range otherwise
 * (8 x 2); any other layout is OCX_E_UNSUPPORTED.  onepass: 0 the streamed second pass, 1 the
 * closed-form comparator where the kernel certifies it.  regret [B] (device): written for the
 * range's sequences only.  gmax (device, nullable; one 64-bit word the caller initialises,
 * 0 for a fresh maximum): max-folded with the bit pattern of every positive regret of the
 * range, so from 0 it ends as the double max(0.0, max regret).  Synchronises `stream`. */
int ocx_test_alg_range(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                       double eta0, int onepass, int64_t g0, int64_t gn, double* regret,
                       double* gmax, void* stream);

/* One launch of the overlapped pipeline's sub-batch generator over sequences
 * [b_off, b_off + nseq) of the layout: the g(T) sampler's streams _rng(base_seed, T, run0 + b)
 * written into the full batch's tiles (y_bits nullable), every slot outside the range left
 * alone.  form 3: the range launcher at three waves per SIMD (its 128-VGPR instance); form 4:
 * at four (its 96-VGPR instance); form 6: the few-stream range launcher (d = 64 only).  The
 * range must lie inside the G * S sequence slots of the layout (else OCX_E_INVALID, checked
 * here); what the launcher itself rejects — b_off or nseq not a multiple of 4, a layout other
 * than d = 16 / 32 / 64 with P * C = d — comes back as OCX_E_INVALID with nothing launched.
 * Synchronises `stream`. */
int ocx_test_gen_gT_range(const ocx_layout* L, uint64_t base_seed, int64_t run0, int64_t b_off,
                          int64_t nseq, int form, double* z_tiled, double* y_tiled,
                          uint64_t* y_bits, void* stream);

/* One launch of the trailing pipeline's row-range generator: rows [t_off, t_off + nrows) of
 * every sequence of the layout's full-horizon tile, the streams fresh (st_in NULL) or resumed
 * from st_in, the stream after the rows saved to st_out (nullable; a buffer other than st_in).
 * st_in / st_out: caller-owned device buffers of 6 * G * S 64-bit words.  labels = 1: the launch
 * also draws the T labels that follow the sequence's last normal (only meaningful on the range
 * that ends at T); labels = 0 leaves y_tiled alone.  Any layout; any cut points.  A range
 * outside [0, T] is OCX_E_INVALID with nothing launched.  Synchronises `stream`. */
int ocx_test_gen_gT_rows(const ocx_layout* L, uint64_t base_seed, int64_t run0, int64_t t_off,
                         int64_t nrows, const uint64_t* st_in, uint64_t* st_out, int labels,
                         double* z_tiled, double* y_tiled, void* stream);

/* The pipelined FTRL (ftl = 0) / FTL (ftl = 1) kernel's persistent instance — the one a batch
 * of more wave-groups than are resident at once launches, each wave looping over groups w,
 * w + nwaves, ... — on a resident batch of any size, with the number of waves forced to
 * `nwaves` (>= 1), so a test reaches one wave running every group, uneven shares and more
 * waves than groups.  onepass as in ocx_test_alg_range.  regret, cum, comp [B] doubles and
 * closed_out [B] int32 (device; all but regret nullable): bit-identical to
 * ocx_dev_simulate_alg_ex on the same data.  OCX_E_UNSUPPORTED for layouts without a
 * persistent instance (it exists for 8 x 8).  Synchronises `stream`. */
int ocx_test_alg_pipe_persistent(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                                 int ftl, double eta0, int onepass, int64_t nwaves, double* regret,
                                 double* cum, double* comp, int32_t* closed_out, void* stream);
/* The same with the label-bit tile y_bits (nullable): the persistent instance that reads it. */
int ocx_test_alg_pipe_persistent_bits(const ocx_layout* L, const double* z_tiled,
                                      const double* y_tiled, const uint64_t* y_bits, int ftl,
                                      double eta0, int onepass, int64_t nwaves, double* regret,
                                      double* cum, double* comp, int32_t* closed_out,
                                      void* stream);

/* ocx_dev_simulate_alg_etas with the group size forced to `group` (1, 2 or 4) instead of
 * ocx_etas_group's choice, so a test reaches every instantiated form whatever the dispatcher
 * prefers.  OCX_E_UNSUPPORTED where that form is not instantiated for the layout (group 2
 * above 16 coordinates per lane, group 4 above 8).  Asynchronous like the product call. */
int ocx_test_simulate_alg_etas(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                               const double* etas, int64_t M, double* regret, double* cum_loss,
                               double* comp_loss, int32_t* closed_out, int flags, int group,
                               void* stream);

/* ocx_dev_simulate_alg_curve_etas with the group size forced to `group` (1, 2 or 4) instead of
 * ocx_curve_etas_group's choice.  OCX_E_UNSUPPORTED where that form is not instantiated for
 * the layout (group 2 above 16 coordinates per lane, group 4 above 8).  The workspace holds
 * G * K * min(group, M) * 64 * (8 C + 12) bytes.  Asynchronous like the product call. */
int ocx_test_simulate_alg_curve_etas(const ocx_layout* L, const double* z_tiled,
                                     const double* y_tiled, const double* etas, int64_t M,
                                     const int64_t* checkpoints, int64_t K, double* regret,
                                     double* cum_loss, double* comp_loss, int32_t* closed_out,
                                     int flags, int group, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ocx_dev_simulate_smart_thresholds with the group size forced to `group` (1, 2 or 4) instead
 * of ocx_smart_thresholds_group's choice.  OCX_E_UNSUPPORTED where that form is not
 * instantiated for the layout (group 2 above 16 coordinates per lane, group 4 above 8).
 * Asynchronous like the product call. */
int ocx_test_simulate_smart_thresholds(const ocx_layout* L, const double* z_tiled,
                                       const double* y_tiled, const double* thresh, int64_t M,
                                       double eta0, double* regret, int64_t* switch_step,
                                       int flags, unsigned long long* stats, int group,
                                       void* stream);

/* ocx_dev_simulate_smart_curve with the group size forced to `group` (1, 2 or 4) instead of
 * ocx_smart_curve_group's choice.  OCX_E_UNSUPPORTED where that form is not instantiated for
 * the layout (group 2 above 16 coordinates per lane, group 4 above 8).  Asynchronous like the
 * product call. */
int ocx_test_simulate_smart_curve(const ocx_layout* L, const double* z_tiled,
                                  const double* y_tiled, const int64_t* horizons,
                                  const double* thresh, int64_t K, double eta0, double* regret,
                                  int64_t* switch_step, int flags, unsigned long long* stats,
                                  int group, void* stream);

/* The one-wave-per-sequence form of the two SMART sweeps (ocx_smart_wave_cols_kernel), forced:
 * always that kernel, in any layout and at any batch size, in launches of `group` (1, 2, 4 or
 * 8) consecutive columns, instead of the dispatch of ocx_dev_simulate_smart_thresholds /
 * ocx_dev_simulate_smart_curve.  Re-scan mode only (no flags).  Column m is the pair
 * (horizons[m], thresh[b][m]); horizons is a HOST array of M non-decreasing values in [0, T],
 * read at call time, or NULL for the threshold sweep (every horizon T).  thresh, regret and
 * switch_step (nullable) are [B][M] device arrays.  The kernel adds in the reference's order
 * whatever the layout, so a butterfly layout gets the exact modes' bits here.  stats (device
 * [2], nullable): stats[0] += the (sequence, step) pairs whose switch test ran, once per step
 * however many columns of the launch needed it; stats[1] is left alone.  OCX_E_UNSUPPORTED
 * for d > 64.  Asynchronous like the product calls. */
int ocx_test_simulate_smart_wave_cols(const ocx_layout* L, const double* z_tiled,
                                      const double* y_tiled, const int64_t* horizons,
                                      const double* thresh, int64_t M, double eta0,
                                      double* regret, int64_t* switch_step,
                                      unsigned long long* stats, int group, void* stream);

/* ocx_dev_simulate_smart_grid on the lane-group kernel (ocx_smart_grid_kernel) with the group
 * size forced to `group` (1, 2 or 4) instead of the dispatch's choice.  OCX_E_UNSUPPORTED where
 * that form is not instantiated for the layout (group 2 above 16 coordinates per lane, group 4
 * above 8).  Asynchronous like the product call. */
int ocx_test_simulate_smart_grid(const ocx_layout* L, const double* z_tiled,
                                 const double* y_tiled, const double* thresh, int64_t M,
                                 const int64_t* checkpoints, int64_t K, double eta0,
                                 double* regret, int64_t* switch_step, int flags,
                                 unsigned long long* stats, int group, void* stream);

/* The one-wave-per-sequence form of the SMART grid (ocx_smart_wave_grid_kernel), forced: always
 * that kernel, in any layout and at any batch size, in launches of `group` (1, 2, 4 or 8)
 * columns.  Re-scan mode only: flags must be 0.  thresh [B][M], checkpoints [K] int64 and the
 * outputs [B][M][K] are device arrays as in ocx_dev_simulate_smart_grid.  The kernel adds in the
 * reference's order whatever the layout.  stats (device [2], nullable): stats[0] += the
 * (sequence, step) pairs whose switch test ran, once per step however many columns of the
 * launch needed it; stats[1] is left alone.  OCX_E_UNSUPPORTED for d > 64.  Asynchronous like
 * the product call. */
int ocx_test_simulate_smart_wave_grid(const ocx_layout* L, const double* z_tiled,
                                      const double* y_tiled, const double* thresh, int64_t M,
                                      const int64_t* checkpoints, int64_t K, double eta0,
                                      double* regret, int64_t* switch_step, int flags,
                                      unsigned long long* stats, int group, void* stream);

/* ocx_dev_twin32_cols in launches of `group` (1, 2, 4 or 8) consecutive columns instead of
 * ocx_twin32_cols_group's choice, so a test reaches every instantiated width.
 * OCX_E_UNSUPPORTED where group * C > 64 (group 8 above 8 coordinates, group 4 above 16).
 * Asynchronous like the product call. */
int ocx_test_twin32_cols(const ocx_layout* L, const double* z_tiled, const double* y_tiled,
                         int64_t K, const int64_t* horizons, const int32_t* algos, double eta0,
                         const double* thresh, float* result, double* cum_loss, float* comp_loss,
                         int64_t* switch_step, int group, void* stream);

/* Batches that have entered the trailing pipeline (ocx_run_gen_sim_trailing) in this process
 * so far: lets a test assert that a call took that path rather than the sequential loop. */
int64_t ocx_test_trailing_batches(void);

#ifdef __cplusplus
}
#endif
#endif /* OCX_TESTING_H_ */
