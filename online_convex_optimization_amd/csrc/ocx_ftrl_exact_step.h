// ocx_ftrl_exact_step.h — the pieces the fused FTRL / exact-FTL kernel (ocx_ftrl_exact.hip) and
// its curve form (ocx_ftrl_exact_curve.hip) share: the N-way per-sequence totals and one whole
// step of both algorithms on a row.
#pragma once
#include "ocx_device_math.h"
#include "ocx_internal.h"

// N per-sequence totals at once; prod(j, k) is product k of this lane's coordinate j.
// Each total keeps the reference's order (sequential over j, then lane to lane in
// chain mode; lane-local then the butterfly in tree mode).
template <int C, int P, bool CHAIN, int N, class F>
__device__ __forceinline__ void ocx_totals(F&& prod, double (&out)[N], int lane) {
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    if constexpr (!CHAIN || P == 1) {
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] += prod(j, k);
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = ocx_seq_sum<P>(acc[k]);
    } else if constexpr (P < OCX_CHAIN_WIDE_P) {
        const int c = lane % P;
        for (int cc = 0; cc < P; ++cc) {
            if (c == cc) {
#pragma unroll
                for (int j = 0; j < C; ++j)
#pragma unroll
                    for (int k = 0; k < N; ++k) acc[k] += prod(j, k);
            }
            if (cc + 1 < P) {
#pragma unroll
                for (int k = 0; k < N; ++k) acc[k] = ocx_dpp<0x138>(acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = __shfl(acc[k], lane - c + P - 1, 64);
    } else {
        // diagonal chain (ocx_device_math.h): every lane adds, the last lane's is the total
#pragma unroll ocx_chain_unroll(P, C)
        for (int cc = 0; cc < P; ++cc) {
#pragma unroll
            for (int j = 0; j < C; ++j)
#pragma unroll
                for (int k = 0; k < N; ++k) acc[k] += prod(j, k);
            if (cc + 1 < P) {
#pragma unroll
                for (int k = 0; k < N; ++k) acc[k] = ocx_dpp<0x138>(acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = ocx_bcast_last<P>(acc[k], lane);
    }
}

// One step of ocx_ftrl_exact_kernel's first pass on row (z, yv), step t (0-based): FTRL's
// action, loss and update of θ_r (tr), exact FTL's of θ_e (te), the regime flag (`linear`),
// the closed forms' row certificate (`clipped`) and linf's touched coordinates.  The curve
// kernel's step; the parent keeps this text written out in its loop (with the function its
// machine code changes: DESIGN.md §3.14).  Whole wave active (the totals cross lanes).
template <int C, int P, bool CHAIN>
__device__ __forceinline__ void ocx_ftrl_exact_step(double (&tr)[C], double (&te)[C],
                                                    const ocx_d2* z, const double& yv,
                                                    OcxScaleTable& sct, const int64_t& t,
                                                    const double& eta0, const int& norm,
                                                    double& cr, double& ce, bool& linear,
                                                    bool& clipped, uint64_t& touch,
                                                    const int& lane) {
    // FTRL action terms (fast_algorithms.py:52-66), exact-FTL norm, ‖z_t‖²
    const double sc = ocx_ftrl_scale(sct, t + 1, eta0, lane);
    double xr[C];
#pragma unroll
    for (int j = 0; j < C; ++j) xr[j] = sc * tr[j];
    double tot[4];
    ocx_totals<C, P, CHAIN, 4>(
        [&](int j, int k) -> double {
            const double zj = ocx_zj(z, j);
            return k == 0 ? xr[j] * xr[j]
                          : (k == 1 ? zj * xr[j] : (k == 2 ? te[j] * te[j] : zj * zj));
        },
        tot, lane);
    double qr = tot[1];
    if (tot[0] > 1.0) {  // FTRL rescale (rare): x *= 1/‖x‖, q again
        const double f = 1.0 / sqrt(tot[0]);
#pragma unroll
        for (int j = 0; j < C; ++j) xr[j] *= f;
        qr = ocx_zdot<C, P, CHAIN>(z, xr, lane);
    }
    // exact FTL: x = FTL(θ_e) (fast_algorithms.py:37-49 form) for l2, the
    // l1 / linf closed forms otherwise; q = z·x
    double xe[C];
    if (norm == 0) {
        const double sce = -(1.0 / sqrt(tot[2]));
#pragma unroll
        for (int j = 0; j < C; ++j) xe[j] = (tot[2] == 0.0) ? 0.0 : sce * te[j];
    } else {
        ocx_action_exact_poly<C, P>(te, xe, norm, lane);
        linear = linear && !ocx_exact_poly_tie<C, P>(te, touch, norm);
    }
    const double qe = ocx_zdot<C, P, CHAIN>(z, xe, lane);
    const double dr = qr - yv;
    cr += 0.5 * fabs(dr);
    ce += 0.5 * fabs(qe - yv);
    if (norm == 0) {
        linear = linear && tot[3] <= 1.0 + 1e-6 && fabs(yv) == 1.0;
    } else {
        linear = linear && ocx_dual_ok<C, P, CHAIN>(z, norm, lane) && fabs(yv) == 1.0;
        if (norm == 2) touch = ocx_touch<C>(touch, z);
    }
    clipped = clipped && tot[3] <= 1.0 + 1e-12;
    const double gr = ocx_grad(dr);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const double zj = ocx_zj(z, j);
        tr[j] += gr * zj;
        te[j] += (-yv) * zj;
    }
}
