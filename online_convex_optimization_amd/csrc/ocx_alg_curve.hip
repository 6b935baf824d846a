// ocx_alg_curve.hip — regret curves: FTRL/FTL (fast_algorithms.py:88-115) observed at K
// checkpoint horizons t_1 < … < t_K <= T in one pass over a sequence of T steps.
//
// FTRL and FTL are online: the first t steps of a run on (z, y) are the run on
// (z[:t], y[:t]).  So the loop of a whole-horizon run passes through the state every
// truncated run would end in, and a curve needs only that the loop stops there and
// evaluates the comparator of the prefix: the loss of FTL(θ_t) over rows 0 … t-1
// (fast_algorithms.py:113-115 applied to the prefix).
//
// Two loop kernels, the curve forms of ocx_alg_kernel (ocx_sim.hip) and of the pipelined
// butterfly kernel (ocx_alg_pipe.hip), dispatched by ocx_launch_alg's rule.  Their step
// arithmetic is that of the kernels they are derived from, operation for operation, so column
// k of a curve carries the bits of a run of those kernels on the input truncated at t_k.
// The checkpoint list is wave-uniform: the kernels hold the next checkpoint in a scalar and
// compare it with the step counter once per step.  At the top of step t == t_k, once `th`
// holds θ_{t_k} (the plain kernel: as the step begins; the pipelined kernel: right after its
// lagging θ is brought up to date), they emit
//   - cum, the loss paid in steps 0 … t_k - 1;
//   - the certificate so far (`clean`: rows in the ball, labels ±1, sub-gradients −y/2);
//   - where the closed form is requested and certified, t_k/2 − ||θ_{t_k}||, the norm summed
//     afresh from θ as the parents' epilogues do.
// t_k = T is emitted after the loop.
//
// A pair (sequence, checkpoint) that does not take the closed form still owes the reference's
// streamed comparator pass over its prefix.  The loop does not re-scan (its register ring
// holds the look-ahead rows): it leaves θ_{t_k}, each lane its own C coordinates, and cum in
// the caller's workspace, and ocx_curve_comp_kernel — one wave per (wave-group, checkpoint) —
// streams rows 0 … t_k - 1 with x* = FTL(θ_{t_k}) in the summation order of the parents'
// second passes.  A wave none of whose sequences needs it exits after one 256-byte read, so a
// certified batch reads z once; otherwise the extra reads are the prefixes of the uncertified
// pairs only.  A certified sequence keeps the closed form whatever its wave neighbours do.
//
// Workspace for K checkpoints (ocx_curve_ws_bytes), slot = g·K + k:
//   θ     [G·K][C][64] doubles   word j of lane l at ((slot·C + j)·64 + l): coalesced
//   cum   [G·K][64]    doubles
//   need  [G·K][64]    int32     1: the lane's sequence takes the streamed pass
//
// The checkpoint array lives in device memory and its order is the caller's precondition.
// Whatever it holds, every access stays inside the batch, the outputs and the workspace: the
// emission index k runs over [0, K) exactly once, rows are addressed by the step counter, and
// the comparator pass clamps its horizon to [0, T].
#include <cstdlib>
#include <type_traits>

#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

#ifndef OCX_PIPE_IT32_MAXC  // ocx_alg_pipe.hip's step-counter rule
#define OCX_PIPE_IT32_MAXC 4
#endif

namespace {

struct CurveArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, G;
    int ftl;
    double eta0;
    const int64_t* ck;  // device [K]
    int64_t K;
    double* regret;    // [B][K], each nullable
    double* cum_out;
    double* comp_out;
    int* closed_out;
    int onepass;
    double* ws_theta;
    double* ws_cum;
    int* ws_need;
};

// The checkpoint list is read-only for the kernels' lifetime and indexed wave-uniformly: read
// through the constant address space it is a scalar load, which waits on the scalar counter
// alone.  (As a global load it compiled to a vector load followed by a wait for EVERY
// outstanding vector access — the emission's stores and the ring's look-ahead rows.  Measured,
// the drain was not what an emission costs: DESIGN.md §3.9.)
typedef const int64_t __attribute__((address_space(4))) * curve_ck_ptr;
__device__ __forceinline__ int64_t curve_ck(const int64_t* ck, int64_t k) {
    return ((curve_ck_ptr)ck)[k];
}

// checkpoint k as the loop's step type, wave-uniform: values past the horizon become T + 1
// (never met inside the loop; emitted after it), negative ones 0; none left: T + 1
template <class IT>
__device__ __forceinline__ IT curve_next(const CurveArgs& a, int64_t k) {
    int64_t v = a.T + 1;
    if (k < a.K) {
        v = curve_ck(a.ck, k);
        v = v < 0 ? 0 : (v > a.T ? a.T + 1 : v);
    }
    const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
    const int hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (IT)(int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// Emission of checkpoint k at horizon tk, th = θ_{tk}.  Whole wave active (lane exchanges).
template <int C, int P, bool CHAIN>
__device__ __forceinline__ void curve_emit(const CurveArgs& a, int64_t g, int64_t k, int64_t tk,
                                           const double (&th)[C], double cum, bool clean,
                                           bool live, int64_t b, int c, int lane) {
    const bool closed = a.onepass && (clean || !live);
    double comp = 0.0;
    if (__ballot(closed) != 0) {  // wave-uniform: the sum below crosses lanes
        double p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = th[j] * th[j];
        const double nrm = sqrt(ocx_total<C, P, CHAIN>(p, lane));
        if (closed) comp = 0.5 * (double)tk - nrm;
    }
    const int64_t slot = g * a.K + k;
    a.ws_need[slot * 64 + lane] = closed ? 0 : 1;
    a.ws_cum[slot * 64 + lane] = cum;
    if (__ballot(!closed) != 0) {  // θ for the streamed pass of this wave's uncertified pairs
#pragma unroll
        for (int j = 0; j < C; ++j) a.ws_theta[(slot * C + j) * 64 + lane] = th[j];
    }
    if (c == 0 && live) {
        const int64_t o = b * a.K + k;
        if (a.cum_out) a.cum_out[o] = cum;
        if (a.closed_out) a.closed_out[o] = closed ? 1 : 0;
        if (closed) {  // the others: ocx_curve_comp_kernel
            if (a.comp_out) a.comp_out[o] = comp;
            if (a.regret) a.regret[o] = cum - comp;
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Curve form of ocx_alg_kernel (algo 0 / 1, no caller comparator): every layout the
// pipelined form does not take, the chained exact layouts included.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_alg_curve_kernel(CurveArgs a) {
    constexpr int S = 64 / P;
    constexpr int K2 = C / 2;
    const int lane = threadIdx.x & 63;
    const int64_t g = ocx_wave_id();
    if (g >= a.G) return;
    const int s = lane / P;
    const int c = lane % P;
    const int64_t b = g * S + s;
    const bool live = b < a.B;
    const int64_t T = a.T;
    const int onepass = a.onepass;
    const double eta0 = a.eta0;
    const bool ftl = a.ftl != 0;
    const int64_t tstride = 64;  // ocx_d2 per step within a plane
    const ocx_d2* __restrict__ zp = reinterpret_cast<const ocx_d2*>(a.zt) + g * T * tstride + lane;
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k)
    const double* __restrict__ yp = a.yt + g * T * S + s;
    bool clean = true;  // every row in the ball, every sub-gradient −y_t/2 so far

    double th[C];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = 0.0;

    ocx_d2 zb[NB][K2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], zp + tl * tstride, kst);
        yb[slot] = yp[tl * S];
    };

    double cum = 0.0;
    int64_t k = 0;
    int64_t nxt = curve_next<int64_t>(a, k);
    OcxScaleTable sct;  // FTRL scales, 64 steps at a time
    ocx_ring_loop<NB>(T, load, [&](int u, int64_t t) {
        while (t >= nxt) {  // wave-uniform; th = θ_t here
            curve_emit<C, P, CHAIN>(a, g, k, t, th, cum, clean, live, b, c, lane);
            ++k;
            nxt = curve_next<int64_t>(a, k);
        }
        double x[C];
        double q;  // :105
        if (!ftl) {
            if constexpr (CHAIN && P >= OCX_CHAIN_WIDE_P) {
                const double sc = ocx_ftrl_scale(sct, t + 1, eta0, lane);
                double fr;
                q = ocx_ftrl_q_sc<C, P, CHAIN>(th, zb[u], sc, fr, lane);
            } else {
                const double sc = ocx_ftrl_scale(sct, t + 1, eta0, lane);
                q = ocx_ftrl_act_dot_sc<C, P, CHAIN>(th, zb[u], sc, x, lane);
            }
        } else {
            ocx_action_ftl<C, P, CHAIN>(th, x, lane);
            q = ocx_zdot<C, P, CHAIN>(zb[u], x, lane);
        }
        const double diff = q - yb[u];  // :106-111
        cum += 0.5 * fabs(diff);
        const double gq = ocx_grad(diff);
        // the closed form's certificate, row by row (whole wave active: the test sums across
        // lanes)
        if (ocx_check_rows(onepass)) clean = clean & ocx_row_in_ball<C, P>(zb[u]);
        clean = clean && fabs(yb[u]) == 1.0 && gq == -0.5 * yb[u];
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] += gq * ocx_zj(zb[u], j);  // gq*z is exact
    });
    // t_k = T, and whatever an unordered list left over: θ_T, the parents' epilogue
    while (k < a.K) {
        curve_emit<C, P, CHAIN>(a, g, k, T, th, cum, clean, live, b, c, lane);
        ++k;
    }
}

// ---------------------------------------------------------------------------
// Curve form of the pipelined butterfly kernel (ocx_alg_pipe.hip, whole runs): the step is
// alg_pipe_body's, see there for the lagging state and the lane partials.
// ---------------------------------------------------------------------------
template <int C, int P, int NB, bool FTL, bool RT>
__global__ __launch_bounds__(OCX_BLOCK, 1) void ocx_alg_pipe_curve_kernel(CurveArgs a) {
    static_assert(P >= 2 && NB >= 4, "butterfly layouts, a ring holding z_{t-1} .. z_{t+1}");
    using IT = typename std::conditional<(C <= OCX_PIPE_IT32_MAXC), int, int64_t>::type;
    constexpr int S = 64 / P;
    constexpr int K2 = C / 2;
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)__builtin_amdgcn_readfirstlane((int)ocx_wave_id());
    if (g >= a.G) return;
    const int64_t T = a.T;
    const double eta0 = a.eta0;
    const int s = lane / P;
    const int c = lane % P;
    const int64_t b = g * S + s;
    const bool live = b < a.B;  // padding sequences skip FTL's near-origin re-sum
    const int64_t tstride = 64;  // ocx_d2 per step within a plane
    const ocx_d2* __restrict__ zg = reinterpret_cast<const ocx_d2*>(a.zt) + g * T * tstride;
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k)
    const double* __restrict__ yg = a.yt + g * T * S;

    double th[C];  // θ_{t-1} (lagging one update)
    double gp = 0.0;                                      // g_{t-1}
    double A = 0.0, Bz = 0.0, U = 0.0, V = 0.0, W = 0.0;  // step t's lane partials
    double cum = 0.0;
    bool clean = true;

    ocx_d2 zb[NB][K2];
    double yb[NB];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = 0.0;
#pragma unroll
    for (int kk = 0; kk < K2; ++kk) zb[NB - 1][kk] = ocx_d2{0.0, 0.0};
    auto load = [&](int slot, int64_t tl) {
        const ocx_d2* __restrict__ row = zg + tl * tstride;  // uniform
#pragma unroll
        for (int kk = 0; kk < K2; ++kk) {
#if OCX_LOAD_NT
            zb[slot][kk] = __builtin_nontemporal_load(row + kk * kst + lane);
#else
            zb[slot][kk] = row[kk * kst + lane];
#endif
        }
        yb[slot] = yg[tl * S + s];
    };
    double scv = 0.0;  // −η0/√(t+1+lane) for the 64 steps from the last multiple of 64
    int64_t k = 0;
    IT nxt = curve_next<IT>(a, k);

    ocx_ring_loop<NB, true, IT>(T, load, [&](int u, int64_t t) {
        if ((t & 63) == 0) {
            if constexpr (!FTL) scv = -(eta0 / sqrt((double)(t + 1 + lane)));
            double uu = 0.0;
#pragma unroll
            for (int j = 0; j < C; ++j) uu = __builtin_fma(th[j], th[j], uu);
            U = uu;
        }
        // ---- chain: g_{t-1} → z_t·θ_t, ||θ_t||² → q_t → g_t
        const double zth = __builtin_fma(gp, Bz, A);
        double tth = __builtin_fma(gp, __builtin_fma(gp, W, 2.0 * V), U);
        // θ_t = θ_{t-1} + g_{t-1} z_{t-1} (exact: g is a power of two or 0)
        const ocx_d2* zp1 = zb[(u + NB - 1) % NB];
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = __builtin_fma(gp, ocx_zj(zp1, j), th[j]);
        while ((IT)t >= nxt) {  // wave-uniform; th = θ_t, cum and clean cover steps < t
            curve_emit<C, P, false>(a, g, k, t, th, cum, clean, live, b, c, lane);
            ++k;
            nxt = curve_next<IT>(a, k);
        }
        const double q_raw = ocx_seq_sum<P>(zth);
        double n_raw = ocx_seq_sum<P>(tth);
        double q;
        if constexpr (!FTL) {
            const double sc = ocx_readlane(scv, (int)(t & 63));  // −η0/√(t+1)
            const double qa = sc * q_raw;
            if (RT && __ballot(sc * sc * n_raw >= 1.0 - 1e-12) == 0) {
                q = qa;
            } else {
                const double s_abs = fabs(sc) * sqrt(n_raw > 0.0 ? n_raw : 0.0);
                q = s_abs > 1.0 ? qa * (1.0 / s_abs) : qa;
            }
        } else {
            if (n_raw < 0.25 && live) {  // near θ = 0: re-sum directly
                double p[C];
#pragma unroll
                for (int j = 0; j < C; ++j) p[j] = th[j] * th[j];
                tth = ocx_lane_sum<C>(p);
                n_raw = ocx_seq_sum<P>(tth);
            }
            q = n_raw == 0.0 ? 0.0 : (-(1.0 / sqrt(n_raw))) * q_raw;
        }
        const double yv = yb[u];
        const double diff = q - yv;  // :106-111
        cum += 0.5 * fabs(diff);
        const double gq = ocx_grad(diff);
        clean = clean && fabs(yv) == 1.0 && gq == -0.5 * yv;

        // ---- off the chain: step t+1's lane partials (θ_t is known, g_t is not)
        const ocx_d2* zc = zb[u];
        const ocx_d2* zn = zb[(u + 1) % NB];  // z_{t+1}, in flight since NB-2 steps
        double w = 0.0, an = 0.0, bn = 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const double zj = ocx_zj(zc, j);
            w = __builtin_fma(zj, zj, w);
            an = __builtin_fma(ocx_zj(zn, j), th[j], an);
            bn = __builtin_fma(ocx_zj(zn, j), zj, bn);
        }
        if (ocx_check_rows(a.onepass)) clean = clean & (ocx_seq_sum<P>(w) <= 1.0 + 1e-12);
        V = zth;
        W = w;
        U = tth;
        A = an;
        Bz = bn;
        gp = gq;
    });
    // θ_T = θ_{T-1} + g_{T-1} z_{T-1} (the row loaded again: its ring slot is not known at
    // compile time), then t_k = T with the parent epilogue's arithmetic
    if (T > 0) {
        ocx_d2 zl[K2];
        ocx_load_tile<C>(zl, zg + (T - 1) * tstride + lane, kst);
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = __builtin_fma(gp, ocx_zj(zl, j), th[j]);
    }
    while (k < a.K) {
        curve_emit<C, P, false>(a, g, k, T, th, cum, clean, live, b, c, lane);
        ++k;
    }
}

// ---------------------------------------------------------------------------
// The streamed comparator of the uncertified (sequence, checkpoint) pairs: wave w = g·K + k
// sums ½|z_t·x* − y_t| over rows 0 … t_k - 1 of wave-group g, x* = FTL(θ_{t_k}) from the
// workspace, in the order of the parents' second passes (ocx_total_last per row, step by step;
// ocx_comp_pass2 pairs the same additions).
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_curve_comp_kernel(CurveArgs a) {
    constexpr int S = 64 / P;
    constexpr int K2 = C / 2;
    const int lane = threadIdx.x & 63;
    const int64_t w = ocx_wave_id();
    if (w >= a.G * a.K) return;
    const int64_t g = w / a.K, k = w - g * a.K;
    const bool need = a.ws_need[w * 64 + lane] != 0;
    if (__ballot(need) == 0) return;  // wave-uniform: every pair of this wave is certified
    int64_t tk = curve_ck(a.ck, k);
    tk = tk < 0 ? 0 : (tk > a.T ? a.T : tk);
    const int s = lane / P;
    const int c = lane % P;
    const int64_t b = g * S + s;
    const int64_t T = a.T;
    const int64_t tstride = 64;
    const ocx_d2* __restrict__ zp = reinterpret_cast<const ocx_d2*>(a.zt) + g * T * tstride + lane;
    const int64_t kst = a.G * T * 64;
    const double* __restrict__ yp = a.yt + g * T * S + s;
    double th[C], xs[C];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = a.ws_theta[(w * C + j) * 64 + lane];
    ocx_action_ftl<C, P, CHAIN>(th, xs, lane);
    ocx_d2 zb[NB][K2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], zp + tl * tstride, kst);
        yb[slot] = yp[tl * S];
    };
    double comp = 0.0;
    ocx_ring_loop<NB>(tk, load, [&](int u, int64_t) {
        double p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = ocx_zj(zb[u], j) * xs[j];
        const double q = ocx_total_last<C, P, CHAIN>(p, lane);
        comp += 0.5 * fabs(q - yb[u]);
    });
    comp = ocx_comp_lane_value<P, CHAIN>(comp, lane);
    if (need && c == 0 && b < a.B) {
        const int64_t o = b * a.K + k;
        if (a.comp_out) a.comp_out[o] = comp;
        if (a.regret) a.regret[o] = a.ws_cum[w * 64 + lane] - comp;
    }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
namespace {

template <int C, int P, bool CH>
hipError_t launch_curve_cp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    const int bw = ocx_block_waves(L->G);
    hipLaunchKernelGGL((ocx_alg_curve_kernel<C, P, CH, nb_for(C, P)>), ocx_grid(L->G, bw),
                       dim3(64 * bw), 0, st, a);
    return hipGetLastError();
}

template <int C, int P, bool CH>
hipError_t launch_comp_cp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    const int64_t n = L->G * a.K;
    const int bw = ocx_block_waves(n);
    hipLaunchKernelGGL((ocx_curve_comp_kernel<C, P, CH, nb_for(C, P)>), ocx_grid(n, bw),
                       dim3(64 * bw), 0, st, a);
    return hipGetLastError();
}

// ocx_alg_pipe.hip's choices: four-wave blocks from four groups on, a ring one slot deeper
// than the plain kernel's, the rescale test everywhere but the 8 x 8 full form
template <int C, int P>
hipError_t launch_pipe_curve_cp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    constexpr int NB = nb_for(C, P) + 1 < 4 ? 4 : nb_for(C, P) + 1;
    constexpr bool RT = !(C == 8 && P == 8);
    const int bw = std::getenv("OCX_BLOCK_WAVES") ? ocx_block_waves(L->G) : (L->G >= 4 ? 4 : 1);
    const dim3 grid = ocx_grid(L->G, bw), block(64 * bw);
    if (a.ftl)
        hipLaunchKernelGGL((ocx_alg_pipe_curve_kernel<C, P, NB, true, RT>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((ocx_alg_pipe_curve_kernel<C, P, NB, false, RT>), grid, block, 0, st, a);
    return hipGetLastError();
}

template <int C>
hipError_t launch_pipe_curve_c(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    switch (L->P) {
        case 8: return launch_pipe_curve_cp<C, 8>(L, a, st);
        case 16: return launch_pipe_curve_cp<C, 16>(L, a, st);
        case 32: return launch_pipe_curve_cp<C, 32>(L, a, st);
        case 64:
            if constexpr (C == 16) return launch_pipe_curve_cp<16, 64>(L, a, st);
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pipe_curve(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    switch (L->C) {
        case 4: return launch_pipe_curve_c<4>(L, a, st);
        case 8: return launch_pipe_curve_c<8>(L, a, st);
        case 16: return launch_pipe_curve_c<16>(L, a, st);
        case 32: return launch_pipe_curve_c<32>(L, a, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_plain_curve(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    OCX_DISPATCH(launch_curve_cp, L, a, st)
}

hipError_t launch_curve_comp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    OCX_DISPATCH(launch_comp_cp, L, a, st)
}

}  // namespace

int64_t ocx_curve_ws_bytes(const ocx_layout* L, int64_t K) {
    return L->G * K * 64 * (8 * (int64_t)L->C + 8 + 4);
}

hipError_t ocx_launch_alg_curve(const ocx_layout* L, const double* zt, const double* yt, int ftl,
                                double eta0, const int64_t* ck, int64_t K, double* reg,
                                double* cum, double* comp, int* closed_out, int onepass,
                                void* ws, hipStream_t st) {
    if (L->G == 0 || K <= 0) return hipSuccess;
    CurveArgs a{};
    a.zt = zt;
    a.yt = yt;
    a.B = L->B;
    a.T = L->T;
    a.G = L->G;
    a.ftl = ftl;
    a.eta0 = eta0;
    a.ck = ck;
    a.K = K;
    a.regret = reg;
    a.cum_out = cum;
    a.comp_out = comp;
    a.closed_out = closed_out;
    a.onepass = onepass;
    const int64_t slots = L->G * K * 64;
    a.ws_theta = static_cast<double*>(ws);
    a.ws_cum = a.ws_theta + slots * L->C;
    a.ws_need = reinterpret_cast<int*>(a.ws_cum + slots);
    // ocx_launch_alg's rule (OCX_ALG_NO_PIPE=1: the plain form, for A/B measurements)
    static const bool no_pipe = [] {
        const char* e = std::getenv("OCX_ALG_NO_PIPE");
        return e && std::atoi(e) != 0;
    }();
    hipError_t e = (!no_pipe && ocx_pipe_supported(L)) ? launch_pipe_curve(L, a, st)
                                                       : launch_plain_curve(L, a, st);
    if (e != hipSuccess) return e;
    return launch_curve_comp(L, a, st);
}
