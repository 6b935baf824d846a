// ocx_smart_grid.h — host-side launchers of the SMART regret grids (ocx_smart_grid.hip,
// ocx_smart_wave_grid.hip): M thresholds, each observed at K checkpoint horizons.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ocx.h"

// Lane-group form (ocx_smart_grid.hip): the M thresholds th [B][M] (device) in passes of at most
// `group` (1, 2 or 4; ocx_smart_grid_instance) columns, each pass observed at the K checkpoints
// ck (DEVICE int64 [K], strictly increasing in [0, T]; anything else gives meaningless numbers
// but stays inside the batch and the outputs); reg / sw [B][M][K] (sw nullable), element
// (b, m, k) the bits of ocx_launch_smart_closed on the rows truncated at ck[k].  stats (nullable,
// device [2]) per launch: += re-scanned (sequence, step) pairs, += (sequence, column,
// checkpoint) triples with the closed comparator.  ocx_smart_grid_best_group: the group the
// measurements chose.
bool ocx_smart_grid_instance(const ocx_layout* L, int group);
int ocx_smart_grid_best_group(const ocx_layout* L);
hipError_t ocx_launch_smart_grid(const ocx_layout* L, const double* zt, const double* yt,
                                 const double* th, int64_t M, const int64_t* ck, int64_t K,
                                 double eta0, double* reg, int64_t* sw, int closed_prefix,
                                 int closed_comp, unsigned long long* stats, int group,
                                 hipStream_t st);
// One-wave-per-sequence form (ocx_smart_wave_grid.hip), re-scan mode only, d <= 64 (else
// hipErrorNotSupported): launches of at most `group` (1, 2, 4 or 8) columns, one prefix re-scan
// per step and one comparator scan per checkpoint for all of a launch's columns; the
// reference's summation order in any layout.  stats[0] (nullable) += (sequence, step) pairs
// whose switch test ran, per launch.
bool ocx_smart_wave_grid_instance(int group);
hipError_t ocx_launch_smart_wave_grid(const ocx_layout* L, const double* zt, const double* yt,
                                      const double* th, int64_t M, const int64_t* ck, int64_t K,
                                      double eta0, double* reg, int64_t* sw,
                                      unsigned long long* stats, int group, hipStream_t st);
