// ocx_ftrl_exact_curve.hip — FTRL against exact FTL (exact_ftl_driver.py:157-190) observed at K
// checkpoint horizons t_1 < … < t_K <= T in one pass over a sequence of T steps: the curve form
// of ocx_ftrl_exact_kernel (ocx_ftrl_exact.hip), built like ocx_alg_curve.hip.
//
// Both algorithms of the parent are online — θ_r follows FTRL, θ_e = −S_t exact FTL, both
// cumulative losses are running sums — so the loop of a whole-horizon run passes through the end
// state of every truncated run, and the exact comparator of a prefix is the closed form of
// S_{t_k}, which the loop holds in registers.  Column k of every output carries the bits the
// parent gives on the batch truncated at t_k (same layout, norm and flags).
//
// Loop kernel: its own loop (ocx_ring_loop) over the parent's step (ocx_ftrl_exact_step), run in
// segments between the horizons of a wave-uniform checkpoint list (ocx_curve_ck.h).  Once the
// state is θ_{t_k} — where the top of step t_k would be, or after the last step for t_k = T — it
// emits with the arithmetic of the parent's epilogue:
//   - cum_ftrl, cum_exact so far;
//   - x*_k from θ_e (ocx_action_ftl for l2, ocx_action_exact_poly for l1 / linf);
//   - the prefix's regime flag: `linear` so far, for l1 / linf && no tie at θ_e;
//   - where the closed form is requested and the pair qualifies (onepass, l2, linear, clipped):
//     comp_exact = t_k/2 + ½ x*_k·θ_e and comp_ftl = t_k/2 + ½ FTL(θ_r)·θ_e from the parent's
//     paired ocx_totals<…, 2> call.
//
// A pair (sequence, checkpoint) that does not take the closed form owes the parent's streamed
// pass 2 over rows 0 … t_k − 1.  The loop does not re-scan: it leaves a need flag per lane and,
// when some sequence of the wave needs the pass, θ_e (and θ_r when comp_ftl is asked for) in the
// caller's workspace; ocx_ftrl_exact_curve_comp_kernel — one wave per (wave-group, checkpoint) —
// rebuilds the actions from them and streams the prefix in the parent's pass-2 order.  A wave
// none of whose pairs needs it exits after one 256-byte read.
//
// Workspace for K checkpoints (ocx_ftrl_exact_curve_ws_bytes), slot = g·K + k:
//   θ_e   [G·K][C][64] doubles   word j of lane l at ((slot·C + j)·64 + l): coalesced
//   θ_r   [G·K][C][64] doubles   only with comp_ftl
//   need  [G·K][64]    int32     1: the lane's sequence takes the streamed pass
//
// The checkpoint array lives in device memory and its order is the caller's precondition.
// Whatever it holds, every access stays inside the batch, the outputs and the workspace: the
// emission index k runs over [0, K) exactly once, horizons are clamped to [0, T] and only ever
// move the loop forward, and the comparator pass clamps its horizon the same way.
#include "ocx_alg_step.h"
#include "ocx_curve_ck.h"
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_ftrl_exact_step.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

struct FeCurveArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, d, G;
    double eta0;
    const int64_t* ck;  // device [K]
    int64_t K;
    double* cum_r;  // [B][K]
    double* cum_e;
    double* comp_e;
    double* comp_f;   // nullable
    double* cmp_out;  // [B][K][d], nullable
    int* regime;
    int* closed_out;  // nullable
    int onepass, norm;
    double* ws_te;
    double* ws_tr;  // nullptr without comp_f
    int* ws_need;
};

// Emission of checkpoint k at horizon tk: the parent's epilogue for a run that ends here.
// `linear` by value: the tie test of θ_{tk} belongs to this prefix alone (the step that
// follows makes it again).  Whole wave active (lane exchanges).
template <int C, int P, bool CHAIN>
__device__ __forceinline__ void fe_curve_emit(const FeCurveArgs& a, int64_t g, int64_t k,
                                              int64_t tk, const double (&tr)[C],
                                              const double (&te)[C], double cr, double ce,
                                              bool linear, bool clipped, uint64_t touch,
                                              bool live, int64_t b, int c, int lane) {
    const int norm = a.norm;
    double xs[C];
    if (norm == 0) {
        ocx_action_ftl<C, P, CHAIN>(te, xs, lane);
    } else {
        ocx_action_exact_poly<C, P>(te, xs, norm, lane);
        linear = linear && !ocx_exact_poly_tie<C, P>(te, touch, norm);
    }
    const int64_t o = b * a.K + k;
    if (a.cmp_out != nullptr && live) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int64_t jj = (int64_t)c * C + j;
            if (jj < a.d) a.cmp_out[o * a.d + jj] = xs[j];
        }
    }
    // (l2 only: FTL(θ_r) is a Euclidean unit vector, so its loss needs ‖z_t‖ <= 1)
    const bool closed = a.onepass && norm == 0 && ((linear && clipped) || !live);
    const int64_t slot = g * a.K + k;
    a.ws_need[slot * 64 + lane] = closed ? 0 : 1;
    if (__ballot(!closed) != 0) {  // wave-uniform: θ for the streamed pass of this wave's pairs
#pragma unroll
        for (int j = 0; j < C; ++j) a.ws_te[(slot * C + j) * 64 + lane] = te[j];
        if (a.ws_tr != nullptr) {
#pragma unroll
            for (int j = 0; j < C; ++j) a.ws_tr[(slot * C + j) * 64 + lane] = tr[j];
        }
    }
    double ke = 0.0, kf = 0.0;
    if (__ballot(closed) != 0) {  // wave-uniform: the sums cross lanes
        double xf[C];
        if (a.comp_f != nullptr) {
            ocx_action_ftl<C, P, CHAIN>(tr, xf, lane);
        } else {
#pragma unroll
            for (int j = 0; j < C; ++j) xf[j] = 0.0;
        }
        double q2[2];
        ocx_totals<C, P, CHAIN, 2>(
            [&](int j, int kk) -> double { return te[j] * (kk ? xf[j] : xs[j]); }, q2, lane);
        if (closed) {
            ke = 0.5 * (double)tk + 0.5 * q2[0];
            kf = 0.5 * (double)tk + 0.5 * q2[1];
        }
    }
    if (c == 0 && live) {
        a.cum_r[o] = cr;
        a.cum_e[o] = ce;
        a.regime[o] = linear ? 1 : 0;
        if (a.closed_out != nullptr) a.closed_out[o] = closed ? 1 : 0;
        if (closed) {  // the others: ocx_ftrl_exact_curve_comp_kernel
            a.comp_e[o] = ke;
            if (a.comp_f != nullptr) a.comp_f[o] = kf;
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Curve form of ocx_ftrl_exact_kernel's first pass and epilogue.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_ftrl_exact_curve_kernel(FeCurveArgs a) {
    const int64_t g = ocx_wave_id();
    if (g >= a.G) return;
    const int64_t T = a.T;
    const OcxSeq<P> q(a.zt, a.yt, g, a.B, T, a.G);
    const int lane = q.lane;
    const double eta0 = a.eta0;
    const int norm = a.norm;

    double tr[C], te[C];  // θ_ftrl, θ_exact = −S_t
#pragma unroll
    for (int j = 0; j < C; ++j) tr[j] = te[j] = 0.0;
    bool linear = true;
    uint64_t touch = 0;   // linf: coordinates some row has touched (ocx_exact_poly_tie)
    bool clipped = true;  // every ‖z_t‖² <= 1 + 1e-12 (closed-form comparators)
    double cr = 0.0, ce = 0.0;

    ocx_d2 zb[NB][C / 2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], q.zp + tl * 64, q.kst);
        yb[slot] = q.yp[tl * q.S];
    };

    // The loop runs in segments, one per checkpoint: rows [t0, t_k) through the ring, then the
    // emission.  (With the emission inside the ring's unrolled body — an observer called at
    // every step, as in ocx_alg_curve.hip — this kernel's two θ vectors, the action and the
    // ring did not fit: instances spilled where the parent's do not.  DESIGN.md §3.14.)  A
    // segment's look-ahead stops at its last row, so a restart costs one load latency per
    // checkpoint, and rows past the last checkpoint are never read.
    int64_t t0 = 0;  // steps done: th = θ_{t0}
    OcxScaleTable sct;  // FTRL scales, 64 steps at a time
    for (int64_t k = 0; k < a.K; ++k) {
        int64_t tk = curve_next<int64_t>(a.ck, a.K, T, k);  // wave-uniform, in [0, T + 1]
        tk = tk > T ? T : tk;
        if (tk > t0) {  // (an unordered list: emitted where the loop stands)
            const int64_t base = t0;
            ocx_ring_loop<NB>(
                tk - base, [&](int slot, int64_t tl) { load(slot, base + tl); },
                [&](int u, int64_t tl) {
                    ocx_ftrl_exact_step<C, P, CHAIN>(tr, te, zb[u], yb[u], sct, base + tl, eta0,
                                                     norm, cr, ce, linear, clipped, touch, lane);
                });
            t0 = tk;
        }
        fe_curve_emit<C, P, CHAIN>(a, g, k, t0, tr, te, cr, ce, linear, clipped, touch, q.live, q.b,
                                   q.c, lane);
    }
}

// ---------------------------------------------------------------------------
// The streamed comparators of the pairs without the closed form: wave w = g·K + k sums
// ½|z_t·x* − y_t| over rows 0 … t_k − 1 of wave-group g — x* from θ_e, and FTL(θ_r) beside it
// when comp_ftl is asked for — in the order of the parent's second pass.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_ftrl_exact_curve_comp_kernel(FeCurveArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = ocx_wave_id();
    if (w >= a.G * a.K) return;
    const int64_t g = w / a.K, k = w - g * a.K;
    const bool need = a.ws_need[w * 64 + lane] != 0;
    if (__ballot(need) == 0) return;  // wave-uniform: every pair of this wave took the closed form
    const int64_t T = a.T;
    int64_t tk = curve_ck(a.ck, k);
    tk = tk < 0 ? 0 : (tk > T ? T : tk);
    const OcxSeq<P> q(a.zt, a.yt, g, a.B, T, a.G);
    const int norm = a.norm;
    double th[C], xs[C], xf[C];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = a.ws_te[(w * C + j) * 64 + lane];
    if (norm == 0) {
        ocx_action_ftl<C, P, CHAIN>(th, xs, lane);
    } else {
        ocx_action_exact_poly<C, P>(th, xs, norm, lane);
    }
    const bool with_f = a.comp_f != nullptr;  // (then ws_tr is there)
    if (with_f) {
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = a.ws_tr[(w * C + j) * 64 + lane];
        ocx_action_ftl<C, P, CHAIN>(th, xf, lane);
    } else {
#pragma unroll
        for (int j = 0; j < C; ++j) xf[j] = 0.0;
    }
    ocx_d2 zb[NB][C / 2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], q.zp + tl * 64, q.kst);
        yb[slot] = q.yp[tl * q.S];
    };
    double ke = 0.0, kf = 0.0;
    if (with_f) {
        ocx_ring_loop<NB>(tk, load, [&](int u, int64_t) {
            const ocx_d2* z = zb[u];
            double q2[2];
            ocx_totals<C, P, CHAIN, 2>(
                [&](int j, int kk) -> double { return ocx_zj(z, j) * (kk ? xf[j] : xs[j]); }, q2,
                lane);
            ke += 0.5 * fabs(q2[0] - yb[u]);
            kf += 0.5 * fabs(q2[1] - yb[u]);
        });
    } else {
        ocx_ring_loop<NB>(tk, load, [&](int u, int64_t) {
            ke += 0.5 * fabs(ocx_zdot<C, P, CHAIN>(zb[u], xs, lane) - yb[u]);
        });
    }
    if (need && q.c == 0 && q.live) {
        const int64_t o = q.b * a.K + k;
        a.comp_e[o] = ke;
        if (with_f) a.comp_f[o] = kf;
    }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
namespace {

template <int C, int P, bool CH>
hipError_t launch_fe_curve_cp(const ocx_layout* L, const FeCurveArgs& a, hipStream_t st) {
    const int bw = ocx_block_waves(L->G);
    hipLaunchKernelGGL((ocx_ftrl_exact_curve_kernel<C, P, CH, nb_for(C, P, false)>),
                       ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
    return hipGetLastError();
}

template <int C, int P, bool CH>
hipError_t launch_fe_comp_cp(const ocx_layout* L, const FeCurveArgs& a, hipStream_t st) {
    const int64_t n = L->G * a.K;
    const int bw = ocx_block_waves(n);
    hipLaunchKernelGGL((ocx_ftrl_exact_curve_comp_kernel<C, P, CH, nb_for(C, P, false)>),
                       ocx_grid(n, bw), dim3(64 * bw), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fe_curve(const ocx_layout* L, const FeCurveArgs& a, hipStream_t st) {
    OCX_DISPATCH(launch_fe_curve_cp, L, a, st)
}

hipError_t launch_fe_comp(const ocx_layout* L, const FeCurveArgs& a, hipStream_t st) {
    OCX_DISPATCH(launch_fe_comp_cp, L, a, st)
}

}  // namespace

int64_t ocx_ftrl_exact_curve_ws_bytes(const ocx_layout* L, int64_t K, int with_comp_f) {
    return L->G * K * 64 * (8 * (int64_t)L->C * (with_comp_f ? 2 : 1) + 4);
}

hipError_t ocx_launch_ftrl_exact_curve(const ocx_layout* L, const double* zt, const double* yt,
                                       double eta0, const int64_t* ck, int64_t K, double* cum_r,
                                       double* cum_e, double* comp_e, double* comp_f,
                                       double* cmp_out, int* regime, int* closed_out, int onepass,
                                       int norm, void* ws, hipStream_t st) {
    if (L->G == 0 || K <= 0) return hipSuccess;
    FeCurveArgs a{};
    a.zt = zt;
    a.yt = yt;
    a.B = L->B;
    a.T = L->T;
    a.d = L->d;
    a.G = L->G;
    a.eta0 = eta0;
    a.ck = ck;
    a.K = K;
    a.cum_r = cum_r;
    a.cum_e = cum_e;
    a.comp_e = comp_e;
    a.comp_f = comp_f;
    a.cmp_out = cmp_out;
    a.regime = regime;
    a.closed_out = closed_out;
    a.onepass = onepass;
    a.norm = norm;
    const int64_t slots = L->G * K * 64;
    a.ws_te = static_cast<double*>(ws);
    a.ws_tr = comp_f != nullptr ? a.ws_te + slots * L->C : nullptr;
    a.ws_need = reinterpret_cast<int*>(a.ws_te + slots * L->C * (comp_f != nullptr ? 2 : 1));
    hipError_t e = launch_fe_curve(L, a, st);
    if (e != hipSuccess) return e;
    return launch_fe_comp(L, a, st);
}
