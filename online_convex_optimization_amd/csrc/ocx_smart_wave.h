// ocx_smart_wave.h — what the two one-wave-per-sequence SMART kernels (ocx_smart_wave.hip,
// ocx_smart_wave_cols.hip) share as code: the ordered adder through LDS that makes them add in
// the reference's order, the sub-gradient, the FTL action and the depth of the speculation.
// The prefix scans (prefix_loss, prefix_loss_multi) and the readlane addressing under them are
// still written out in both files: moved here they change the device assembly (DESIGN.md
// §3.13).
#pragma once
#include "ocx_internal.h"

namespace {

constexpr int kSpec = 4;  // pre-switch steps whose prefix re-scans run side by side

// acc + v_0 + v_1 + ... + v_{n-1}, left to right (v_k = lane k's value), n <= 64.
// The values go through the wave's LDS slot `buf`; every lane returns the same sum.
__device__ __forceinline__ double ordered_sum(double acc, double v, int n, double* buf,
                                              int lane) {
    buf[lane] = v;
    __builtin_amdgcn_wave_barrier();
    int k = 0;
    for (; k + 8 <= n; k += 8) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = buf[k + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += t[u];
    }
    for (; k < n; ++k) acc += buf[k];
    __builtin_amdgcn_wave_barrier();
    return acc;
}

__device__ __forceinline__ double grad(double diff) {
    return diff > 0.0 ? 0.5 : (diff < 0.0 ? -0.5 : 0.0);
}

// FTL action (fast_algorithms.py:37-49) of the d-coordinate state of which this lane holds
// coordinate `lane` in `th` (lanes >= d hold none)
__device__ __forceinline__ double action_ftl(double th, int d, double* buf, int lane) {
    const double n2 = ordered_sum(0.0, lane < d ? th * th : 0.0, d, buf, lane);
    if (n2 == 0.0) return 0.0;
    const double scale = -(1.0 / sqrt(n2));
    return scale * th;
}

}  // namespace
