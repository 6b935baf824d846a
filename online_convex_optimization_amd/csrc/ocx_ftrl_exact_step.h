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

// ocx_ftrl_scale's table for NE step sizes: one base, the √ shared, −(η_m/√t) per column — the
// same expression per (t, m) as OcxScaleTable's, so bit for bit the same scale.
template <int NE>
struct OcxScaleCols {
    double v[NE];
    int64_t base = INT64_MIN / 2;  // 1-based step of lane 0's entries (none yet)
};

// Column form of ocx_ftrl_exact_step (the regret grid's step, ocx_ftrl_exact_grid.hip): NE FTRL
// columns, θ_r^m (tr[m]) at step size eta[m] with its own loss cr[m], beside ONE exact-FTL
// column.  Formed once: the exact action, its q, ‖θ_e‖², ‖z_t‖², the dual-ball and touch tests,
// the θ_e update, `linear` and `clipped`.  Formed per column: the scale, the action, ‖x_r‖²,
// z·x_r, the rescale branch (each column's own test), the loss, the sub-gradient and the θ_r
// update.  Every total is accumulated on its own (ocx_totals), so the 2 + 2·NE wide call keeps
// each one's order, and each column's products and sums are those of the NE = 1 step.
template <int C, int P, bool CHAIN, int NE>
__device__ __forceinline__ void ocx_ftrl_exact_step_cols(
    double (&tr)[NE][C], double (&te)[C], const ocx_d2* z, const double& yv, OcxScaleCols<NE>& sct,
    const int64_t& t, const double (&eta)[NE], const int& norm, double (&cr)[NE], double& ce,
    bool& linear, bool& clipped, uint64_t& touch, const int& lane) {
    const int64_t t1 = t + 1;
    if (t1 - sct.base >= 64 || t1 < sct.base) {
        sct.base = t1;
        const double r = sqrt((double)(t1 + lane));
#pragma unroll
        for (int m = 0; m < NE; ++m) sct.v[m] = -(eta[m] / r);
    }
    double xr[NE][C];
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        const double sc = ocx_readlane(sct.v[m], (int)(t1 - sct.base));
#pragma unroll
        for (int j = 0; j < C; ++j) xr[m][j] = sc * tr[m][j];
    }
    // totals 2m: ‖x_r^m‖², 2m + 1: z·x_r^m; then ‖θ_e‖² and ‖z_t‖²
    double tot[2 * NE + 2];
    ocx_totals<C, P, CHAIN, 2 * NE + 2>(
        [&](int j, int k) -> double {
            const double zj = ocx_zj(z, j);
            if (k == 2 * NE) return te[j] * te[j];
            if (k == 2 * NE + 1) return zj * zj;
            const int m = k >> 1;
            return (k & 1) ? zj * xr[m][j] : xr[m][j] * xr[m][j];
        },
        tot, lane);
    const double te2 = tot[2 * NE], z2 = tot[2 * NE + 1];
    double qr[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        qr[m] = tot[2 * m + 1];
        if (tot[2 * m] > 1.0) {  // FTRL rescale (rare), this column's own test
            const double f = 1.0 / sqrt(tot[2 * m]);
#pragma unroll
            for (int j = 0; j < C; ++j) xr[m][j] *= f;
            qr[m] = ocx_zdot<C, P, CHAIN>(z, xr[m], lane);
        }
    }
    double xe[C];
    if (norm == 0) {
        const double sce = -(1.0 / sqrt(te2));
#pragma unroll
        for (int j = 0; j < C; ++j) xe[j] = (te2 == 0.0) ? 0.0 : sce * te[j];
    } else {
        ocx_action_exact_poly<C, P>(te, xe, norm, lane);
        linear = linear && !ocx_exact_poly_tie<C, P>(te, touch, norm);
    }
    const double qe = ocx_zdot<C, P, CHAIN>(z, xe, lane);
    ce += 0.5 * fabs(qe - yv);
    if (norm == 0) {
        linear = linear && z2 <= 1.0 + 1e-6 && fabs(yv) == 1.0;
    } else {
        linear = linear && ocx_dual_ok<C, P, CHAIN>(z, norm, lane) && fabs(yv) == 1.0;
        if (norm == 2) touch = ocx_touch<C>(touch, z);
    }
    clipped = clipped && z2 <= 1.0 + 1e-12;
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        const double dr = qr[m] - yv;
        cr[m] += 0.5 * fabs(dr);
        const double gr = ocx_grad(dr);
#pragma unroll
        for (int j = 0; j < C; ++j) tr[m][j] += gr * ocx_zj(z, j);
    }
#pragma unroll
    for (int j = 0; j < C; ++j) te[j] += (-yv) * ocx_zj(z, j);
}
