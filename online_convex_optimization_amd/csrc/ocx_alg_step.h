// ocx_alg_step.h — pieces of the FTRL/FTL step (fast_algorithms.py:88-115), each defined once.
//
// Users: alg_pipe_body (ocx_alg_pipe.h), the loop of ocx_alg_pipe_kernel and of its curve form,
// calls the pipelined pieces and ocx_loss_grad / ocx_cert_grad; the plain curve kernel and the
// curve comparator kernel (ocx_alg_curve.hip) call ocx_plain_step, ocx_closed_comp,
// ocx_comp_stream and OcxSeq.  Not users, their step stays written out: ocx_alg_kernel
// (ocx_sim.hip), ocx_alg_chunk_kernel (ocx_stream.hip), the SMART kernel's FTL leg
// (ocx_smart_thresholds.hip; measured on its former single-threshold twin) — with any of
// these pieces their machine code changes — and the step-size kernels (ocx_alg_etas.hip), which
// measured slower built from them.  DESIGN.md §3.9, "Shared step", has the figures.
//
// Scalar inputs are taken by const&, not by value: the reads then stay where the written-out
// code had them (inside short-circuit blocks), which keeps alg_pipe_body's code unchanged.
#pragma once
#include "ocx_device_math.h"
#include "ocx_internal.h"

// ---------------------------------------------------------------------------
// Prologue: where this lane of wave-group g finds its sequence and its rows.  Row t of the
// group: pair k of this lane at zp[t * 64 + k * kst], the label at yp[t * S].
// ---------------------------------------------------------------------------
template <int P>
struct OcxSeq {
    static constexpr int S = 64 / P;
    int lane, s, c;
    int64_t b;  // the sequence
    bool live;  // b < B: not one of the layout's padding sequences
    const ocx_d2* __restrict__ zp;
    int64_t kst;  // plane stride (pairs k)
    const double* __restrict__ yp;
    __device__ __forceinline__ OcxSeq(const double* zt, const double* yt, int64_t g, int64_t B,
                                      int64_t T, int64_t G)
        : lane(threadIdx.x & 63), s(lane / P), c(lane % P), b(g * S + s), live(b < B),
          zp(reinterpret_cast<const ocx_d2*>(zt) + g * T * 64 + lane), kst(G * T * 64),
          yp(yt + g * T * S + s) {}
};

// ---------------------------------------------------------------------------
// Loss, sub-gradient, certificate: both steps
// ---------------------------------------------------------------------------
// ½|q − y| added to cum; returns g_t (fast_algorithms.py:106-111)
__device__ __forceinline__ double ocx_loss_grad(const double& q, const double& y, double& cum) {
    const double diff = q - y;
    cum += 0.5 * fabs(diff);
    return ocx_grad(diff);
}

// The closed form's certificate, label and sub-gradient part: y_t = ±1 and g_t = −y_t/2 (then
// θ_T = −½ Σ y_t z_t exactly).  The row part (||z_t|| <= 1): ocx_row_in_ball, ocx_pipe_advance.
// UNIT: y was formed as ±1.0 from a label bit (ocx_alg_pipe.h, BITS), so |y| = 1 holds by
// construction and only the sub-gradient is tested.
template <bool UNIT = false>
__device__ __forceinline__ void ocx_cert_grad(bool& clean, const double& y, const double& gq) {
    if constexpr (UNIT) clean = clean && gq == -0.5 * y;
    else clean = clean && fabs(y) == 1.0 && gq == -0.5 * y;
}

// ---------------------------------------------------------------------------
// The plain step
// ---------------------------------------------------------------------------
// One whole plain step of algo 0 / 1 on row (z, y): q_t (:105), loss, certificate, θ update
// (g z is exact: g is 0 or ±½).  scale() gives FTRL's −η0/√(t+1) and is called on the FTRL
// branch only.  check: certify the row inside the unit ball too (whole wave active: the test
// sums across lanes).
template <int C, int P, bool CHAIN, class Scale>
__device__ __forceinline__ void ocx_plain_step(bool ftl, double (&th)[C], const ocx_d2* z,
                                               double y, bool check, double& cum, bool& clean,
                                               int lane, Scale&& scale) {
    double x[C];
    double q;
    if (!ftl) {
        if constexpr (CHAIN && P >= OCX_CHAIN_WIDE_P) {
            double fr;
            q = ocx_ftrl_q_sc<C, P, CHAIN>(th, z, scale(), fr, lane);
        } else {
            q = ocx_ftrl_act_dot_sc<C, P, CHAIN>(th, z, scale(), x, lane);
        }
    } else {
        ocx_action_ftl<C, P, CHAIN>(th, x, lane);
        q = ocx_zdot<C, P, CHAIN>(z, x, lane);
    }
    const double gq = ocx_loss_grad(q, y, cum);
    if (check) clean = clean & ocx_row_in_ball<C, P>(z);
    ocx_cert_grad(clean, y, gq);
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] += gq * ocx_zj(z, j);
}

// ---------------------------------------------------------------------------
// The pipelined step (ocx_alg_pipe.h)
// ---------------------------------------------------------------------------
// Every 64 steps (t a multiple of 64): the FTRL scales −η0/√(t+1+lane) of the next 64 steps
// (one per lane, one sqrt/div per lane instead of one per step) and ||θ||²'s lane part summed
// afresh, so the running update drifts for at most 64 steps.
template <bool FTL, int C>
__device__ __forceinline__ void ocx_pipe_refresh(int64_t t, int lane, const double& eta0,
                                                 double& scv, const double (&th)[C], double& U) {
    if constexpr (!FTL) scv = -(eta0 / sqrt((double)(t + 1 + lane)));
    double uu = 0.0;
#pragma unroll
    for (int j = 0; j < C; ++j) uu = __builtin_fma(th[j], th[j], uu);
    U = uu;
}

// FTRL's q from z_t·θ_t and ||θ_t||² (summed over the sequence's lanes), sc = −η/√(t+1).
// RT: no sequence of the wave near the rescale (s²||θ||² < 1 − 1e-12, far outside the rounding
// of the test below): q = s·(z·θ), without the sqrt the test below needs — what the test below
// would give, bit for bit.  On the g(T) rows ||sθ|| stays near 0.71 and the rescale is rare
// (DESIGN §3.1).
template <bool RT>
__device__ __forceinline__ double ocx_pipe_q_ftrl(const double& sc, const double& q_raw,
                                                  const double& n_raw) {
    const double qa = sc * q_raw;
    if (RT && __ballot(sc * sc * n_raw >= 1.0 - 1e-12) == 0) return qa;
    const double s_abs = fabs(sc) * sqrt(n_raw > 0.0 ? n_raw : 0.0);
    return s_abs > 1.0 ? qa * (1.0 / s_abs) : qa;
}

// FTL's q.  Near θ = 0, where the running ||θ_t||² would lose relative accuracy to
// cancellation, it is re-summed directly (tth, n_raw replaced) — by the live sequences: a
// padding sequence's θ stays 0 and would re-sum at every step.
template <int C, int P>
__device__ __forceinline__ double ocx_pipe_q_ftl(const double (&th)[C], const double& q_raw,
                                                 double& n_raw, double& tth, const bool& live) {
    if (n_raw < 0.25 && live) {
        double p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = th[j] * th[j];
        tth = ocx_lane_sum<C>(p);
        n_raw = ocx_seq_sum<P>(tth);
    }
    return n_raw == 0.0 ? 0.0 : (-(1.0 / sqrt(n_raw))) * q_raw;
}

// Off the chain: step t+1's lane partials (θ_t is known, g_t is not) from z_t (zc) and
// z_{t+1} (zn), the certificate's row test from W, and the state handed on to step t+1.
// (At t = T-1, zn is the clamped look-ahead: A and Bz are then never used.)
template <int P, int C>
__device__ __forceinline__ void ocx_pipe_advance(const double (&th)[C], const ocx_d2* zc,
                                                 const ocx_d2* zn, int onepass, const double& zth,
                                                 const double& tth, const double& gq, double& A,
                                                 double& Bz, double& U, double& V, double& W,
                                                 double& gp, bool& clean) {
    double w = 0.0, an = 0.0, bn = 0.0;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        const double zj = ocx_zj(zc, j);
        w = __builtin_fma(zj, zj, w);
        an = __builtin_fma(ocx_zj(zn, j), th[j], an);
        bn = __builtin_fma(ocx_zj(zn, j), zj, bn);
    }
    // row t in the ball
    if (ocx_check_rows(onepass)) clean = clean & (ocx_seq_sum<P>(w) <= 1.0 + 1e-12);
    V = zth;
    W = w;
    U = tth;  // ||θ_t||²'s lane part, by the running update
    A = an;
    Bz = bn;
    gp = gq;
}

// ---------------------------------------------------------------------------
// Epilogue: the comparator FTL(θ_t) of a prefix of t rows (fast_algorithms.py:113-115)
// ---------------------------------------------------------------------------
// Closed form t/2 − ||θ_t|| for the lanes with `closed` set, the norm summed afresh from θ.
// The sum crosses lanes, so the whole wave runs it when any lane asks (wave-uniform ballot).
template <int C, int P, bool CHAIN>
__device__ __forceinline__ void ocx_closed_comp(const double (&th)[C], const bool& closed,
                                                const int64_t& t, double& comp, const int& lane) {
    if (__ballot(closed) != 0) {
        double p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = th[j] * th[j];
        const double nrm = sqrt(ocx_total<C, P, CHAIN>(p, lane));
        if (closed) comp = 0.5 * (double)t - nrm;
    }
}

// The streamed second pass over rows [0, T) through the kernel's own ring (zb, yb, load):
// Σ ½|z_t·x* − y_t| (:69-76); the long chains leave it in the sequence's last lane.
template <int C, int P, bool CHAIN, int NB, class Load>
__device__ __forceinline__ double ocx_comp_stream(int64_t T, Load&& load,
                                                  ocx_d2 (&zb)[NB][C / 2], double (&yb)[NB],
                                                  const double (&xs)[C], int lane) {
    double comp = 0.0;
    ocx_ring_loop<NB>(T, load, [&](int u, int64_t) {
        double p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = ocx_zj(zb[u], j) * xs[j];
        const double q = ocx_total_last<C, P, CHAIN>(p, lane);
        comp += 0.5 * fabs(q - yb[u]);
    });
    return ocx_comp_lane_value<P, CHAIN>(comp, lane);
}
