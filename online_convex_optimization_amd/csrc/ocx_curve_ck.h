// ocx_curve_ck.h — the checkpoint list of the curve kernels (ocx_alg_curve.hip,
// ocx_ftrl_exact_curve.hip): a device int64 array [K] that every wave walks once, in order.
#pragma once
#include "ocx_internal.h"

// The checkpoint list is read-only for the kernels' lifetime and indexed wave-uniformly: read
// through the constant address space it is a scalar load, which waits on the scalar counter
// alone.  (As a global load it compiled to a vector load followed by a wait for EVERY
// outstanding vector access — the emission's stores and the ring's look-ahead rows.  Measured,
// the drain was not what an emission costs: DESIGN.md §3.9.)
typedef const int64_t __attribute__((address_space(4))) * curve_ck_ptr;
__device__ __forceinline__ int64_t curve_ck(const int64_t* ck, int64_t k) {
    return ((curve_ck_ptr)ck)[k];
}

// checkpoint k of ck[K] as the loop's step type, wave-uniform: values past the horizon T become
// T + 1 (never met inside the loop; emitted after it), negative ones 0; none left: T + 1
template <class IT>
__device__ __forceinline__ IT curve_next(const int64_t* ck, int64_t K, int64_t T, int64_t k) {
    int64_t v = T + 1;
    if (k < K) {
        v = curve_ck(ck, k);
        v = v < 0 ? 0 : (v > T ? T + 1 : v);
    }
    const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const int hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (IT)(int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
