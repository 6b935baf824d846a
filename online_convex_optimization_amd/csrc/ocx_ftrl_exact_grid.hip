// ocx_ftrl_exact_grid.hip — FTRL against exact FTL (exact_ftl_driver.py:157-190) for NE values
// of eta0, each observed at K checkpoint horizons t_1 < … < t_K <= T, in one pass over z: the
// step-size form of ocx_ftrl_exact_curve.hip, built the way ocx_alg_curve_etas.hip is built from
// ocx_alg_curve.hip.
//
// Of the two loops of the parent's step only FTRL depends on eta0.  The loop kernel holds the
// exact side once per sequence — θ_e, exact FTL's loss, `linear`, `clipped`, `touch` — and the
// FTRL side NE times (θ_r^m, its loss; NE = 1, 2, 4); every z_t / y_t row is loaded once per
// step for all of them (ocx_ftrl_exact_step_cols, ocx_ftrl_exact_step.h).  Element (b, m, k) of
// cum_ftrl / comp_ftl and element (b, k) of cum_exact / comp_exact / regime / closed /
// cmp_action carry the bits of ocx_ftrl_exact_curve_kernel with eta0 = etas[m] at column k
// (same layout, norm and flags): each column's arithmetic is the parent's, operation for
// operation, and every sum is taken on its own in the parent's order.
//
// Segments as in the parent: rows [t_{k-1}, t_k) go through ocx_ring_loop, the emission happens
// outside the ring.  The emission is the parent's epilogue (fe_curve_emit) with the exact side
// formed once — x*_k, the regime flag, `closed`, comp_exact, cum_exact, cmp_action — and per
// column cum_ftrl and, where asked for, comp_ftl = t_k/2 + ½ FTL(θ_r^m)·θ_e.  `closed` does not
// depend on eta0: onepass && l2 && linear && clipped.
//
// A pair (sequence, checkpoint) that does not take the closed form owes the streamed pass over
// rows 0 … t_k − 1.  ocx_ftrl_exact_grid_comp_kernel — one wave per (wave-group, checkpoint) —
// exits after the 256-byte need read when no pair of the wave needs it, and otherwise streams
// the prefix once for x* and for FTL(θ_r^m) of every column of the launch.
//
// Workspace of one launch of ne columns (ocx_ftrl_exact_grid_ws_bytes sizes it for the largest
// launch; the next group of step sizes reuses it, in stream order), slot = g·K + k:
//   θ_e   [G·K][C][64]    doubles   word j of lane l at ((slot·C + j)·64 + l): coalesced
//   θ_r   [G·K·ne][C][64] doubles   only with comp_ftl; column m at slot·ne + m
//   need  [G·K][64]       int32     1: the lane's sequence takes the streamed pass
//
// The checkpoint array lives in device memory and its order is the caller's precondition.
// Whatever it holds, every access stays inside the batch, the outputs and the workspace: the
// emission index k runs over [0, K) exactly once, horizons are clamped to [0, T] and only ever
// move the loop forward, and the comparator pass clamps its horizon the same way.
//
// The step sizes travel in the kernel arguments.  η-dependent outputs are [B][M][K], this
// launch's columns m0 … m0 + ne − 1; a launch may hold fewer columns than its instance
// (ne < NE): the spare column runs on a copy of the last step size and writes nothing.  Every
// launch re-runs the exact side; the η-independent outputs are written by the first alone.
#include "ocx_alg_step.h"
#include "ocx_curve_ck.h"
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_ftrl_exact_step.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

constexpr int kMaxNE = 4;

struct FeGridArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, d, G;
    double eta[kMaxNE];
    int ne;          // columns of this launch (<= the instance's NE)
    int64_t M, m0;   // step sizes of the call, first column of this launch
    const int64_t* ck;  // device [K]
    int64_t K;
    double* cum_r;    // [B][M][K]
    double* comp_f;   // [B][M][K], nullable
    double* cum_e;    // [B][K]: these five by the launch with m0 == 0 only
    double* comp_e;
    double* cmp_out;  // [B][K][d], nullable
    int* regime;
    int* closed_out;  // nullable
    int onepass, norm;
    double* ws_te;
    double* ws_tr;  // nullptr without comp_f
    int* ws_need;
};

// Emission of checkpoint k at horizon tk: fe_curve_emit (ocx_ftrl_exact_curve.hip) with the
// exact side formed once and the FTRL side per column.  `linear` by value: the tie test of
// θ_{tk} belongs to this prefix alone.  Whole wave active (lane exchanges).
template <int C, int P, bool CHAIN, int NE>
__device__ __forceinline__ void fe_grid_emit(const FeGridArgs& a, int64_t g, int64_t k, int64_t tk,
                                             const double (&tr)[NE][C], const double (&te)[C],
                                             const double (&cr)[NE], double ce, bool linear,
                                             bool clipped, uint64_t touch, bool live, int64_t b,
                                             int c, int lane) {
    const int norm = a.norm;
    const bool first = a.m0 == 0;
    double xs[C];
    if (norm == 0) {
        ocx_action_ftl<C, P, CHAIN>(te, xs, lane);
    } else {
        ocx_action_exact_poly<C, P>(te, xs, norm, lane);
        linear = linear && !ocx_exact_poly_tie<C, P>(te, touch, norm);
    }
    const int64_t o = b * a.K + k;
    if (first && a.cmp_out != nullptr && live) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const int64_t jj = (int64_t)c * C + j;
            if (jj < a.d) a.cmp_out[o * a.d + jj] = xs[j];
        }
    }
    const bool closed = a.onepass && norm == 0 && ((linear && clipped) || !live);
    const int64_t slot = g * a.K + k;
    a.ws_need[slot * 64 + lane] = closed ? 0 : 1;
    if (__ballot(!closed) != 0) {  // wave-uniform: θ for the streamed pass of this wave's pairs
#pragma unroll
        for (int j = 0; j < C; ++j) a.ws_te[(slot * C + j) * 64 + lane] = te[j];
        if (a.ws_tr != nullptr) {
#pragma unroll
            for (int m = 0; m < NE; ++m) {
                if (m < a.ne) {  // wave-uniform
#pragma unroll
                    for (int j = 0; j < C; ++j)
                        a.ws_tr[((slot * a.ne + m) * C + j) * 64 + lane] = tr[m][j];
                }
            }
        }
    }
    double ke = 0.0;
    double kf[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) kf[m] = 0.0;
    if (__ballot(closed) != 0) {  // wave-uniform: the sums cross lanes
        // the parent's paired call per column: q2[0] = θ_e·x* is the same sum each time
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            if (m == 0 || (a.comp_f != nullptr && m < a.ne)) {  // wave-uniform
                double xf[C];
                if (a.comp_f != nullptr) {
                    ocx_action_ftl<C, P, CHAIN>(tr[m], xf, lane);
                } else {
#pragma unroll
                    for (int j = 0; j < C; ++j) xf[j] = 0.0;
                }
                double q2[2];
                ocx_totals<C, P, CHAIN, 2>(
                    [&](int j, int kk) -> double { return te[j] * (kk ? xf[j] : xs[j]); }, q2,
                    lane);
                if (closed) {
                    if (m == 0) ke = 0.5 * (double)tk + 0.5 * q2[0];
                    kf[m] = 0.5 * (double)tk + 0.5 * q2[1];
                }
            }
        }
    }
    if (c == 0 && live) {
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            if (m < a.ne) {
                const int64_t om = (b * a.M + a.m0 + m) * a.K + k;
                a.cum_r[om] = cr[m];
                if (closed && a.comp_f != nullptr) a.comp_f[om] = kf[m];
            }
        }
        if (first) {
            a.cum_e[o] = ce;
            a.regime[o] = linear ? 1 : 0;
            if (a.closed_out != nullptr) a.closed_out[o] = closed ? 1 : 0;
            if (closed) a.comp_e[o] = ke;  // the others: ocx_ftrl_exact_grid_comp_kernel
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Step-size form of ocx_ftrl_exact_curve_kernel.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB, int NE>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_ftrl_exact_grid_kernel(FeGridArgs a) {
    const int64_t g = ocx_wave_id();
    if (g >= a.G) return;
    const int64_t T = a.T;
    const OcxSeq<P> q(a.zt, a.yt, g, a.B, T, a.G);
    const int lane = q.lane;
    const int norm = a.norm;
    double eta[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) eta[m] = a.eta[m];

    double tr[NE][C], te[C];  // θ_ftrl per column, θ_exact = −S_t
    double cr[NE];
#pragma unroll
    for (int j = 0; j < C; ++j) te[j] = 0.0;
#pragma unroll
    for (int m = 0; m < NE; ++m) {
#pragma unroll
        for (int j = 0; j < C; ++j) tr[m][j] = 0.0;
        cr[m] = 0.0;
    }
    bool linear = true;
    uint64_t touch = 0;
    bool clipped = true;
    double ce = 0.0;

    ocx_d2 zb[NB][C / 2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], q.zp + tl * 64, q.kst);
        yb[slot] = q.yp[tl * q.S];
    };

    int64_t t0 = 0;  // steps done
    OcxScaleCols<NE> sct;
    for (int64_t k = 0; k < a.K; ++k) {
        int64_t tk = curve_next<int64_t>(a.ck, a.K, T, k);  // wave-uniform, in [0, T + 1]
        tk = tk > T ? T : tk;
        if (tk > t0) {  // (an unordered list: emitted where the loop stands)
            const int64_t base = t0;
            ocx_ring_loop<NB>(
                tk - base, [&](int slot, int64_t tl) { load(slot, base + tl); },
                [&](int u, int64_t tl) {
                    ocx_ftrl_exact_step_cols<C, P, CHAIN, NE>(tr, te, zb[u], yb[u], sct, base + tl,
                                                              eta, norm, cr, ce, linear, clipped,
                                                              touch, lane);
                });
            t0 = tk;
        }
        fe_grid_emit<C, P, CHAIN, NE>(a, g, k, t0, tr, te, cr, ce, linear, clipped, touch, q.live,
                                      q.b, q.c, lane);
    }
}

// ---------------------------------------------------------------------------
// The streamed comparators of the pairs without the closed form: wave w = g·K + k sums
// ½|z_t·x − y_t| over rows 0 … t_k − 1 of wave-group g once — for x* from θ_e and, when comp_ftl
// is asked for, FTL(θ_r^m) of every column of the launch beside it — each sum in the order of
// ocx_ftrl_exact_curve_comp_kernel.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB, int NE>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_ftrl_exact_grid_comp_kernel(FeGridArgs a) {
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
    const bool first = a.m0 == 0;
    double th[C], xs[C];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = a.ws_te[(w * C + j) * 64 + lane];
    if (norm == 0) {
        ocx_action_ftl<C, P, CHAIN>(th, xs, lane);
    } else {
        ocx_action_exact_poly<C, P>(th, xs, norm, lane);
    }
    ocx_d2 zb[NB][C / 2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], q.zp + tl * 64, q.kst);
        yb[slot] = q.yp[tl * q.S];
    };
    const bool with_f = a.comp_f != nullptr;  // (then ws_tr is there)
    if (with_f) {
        double xf[NE][C];
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            if (m < a.ne) {  // wave-uniform
#pragma unroll
                for (int j = 0; j < C; ++j)
                    th[j] = a.ws_tr[((w * a.ne + m) * C + j) * 64 + lane];
                ocx_action_ftl<C, P, CHAIN>(th, xf[m], lane);
            } else {
#pragma unroll
                for (int j = 0; j < C; ++j) xf[m][j] = 0.0;
            }
        }
        double kk[NE + 1];
#pragma unroll
        for (int n = 0; n <= NE; ++n) kk[n] = 0.0;
        ocx_ring_loop<NB>(tk, load, [&](int u, int64_t) {
            const ocx_d2* z = zb[u];
            double qn[NE + 1];
            ocx_totals<C, P, CHAIN, NE + 1>(
                [&](int j, int n) -> double {
                    return ocx_zj(z, j) * (n == 0 ? xs[j] : xf[n == 0 ? 0 : n - 1][j]);
                },
                qn, lane);
#pragma unroll
            for (int n = 0; n <= NE; ++n) kk[n] += 0.5 * fabs(qn[n] - yb[u]);
        });
        if (need && q.c == 0 && q.live) {
            if (first) a.comp_e[q.b * a.K + k] = kk[0];
#pragma unroll
            for (int m = 0; m < NE; ++m) {
                if (m < a.ne) a.comp_f[(q.b * a.M + a.m0 + m) * a.K + k] = kk[m + 1];
            }
        }
    } else {
        if (!first) return;  // the exact comparator is the first launch's
        double ke = 0.0;
        ocx_ring_loop<NB>(tk, load, [&](int u, int64_t) {
            ke += 0.5 * fabs(ocx_zdot<C, P, CHAIN>(zb[u], xs, lane) - yb[u]);
        });
        if (need && q.c == 0 && q.live) a.comp_e[q.b * a.K + k] = ke;
    }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
namespace {

// NE = 1 for every layout.  NE = 2 and 4 where the loop kernel has no scratch beside an NE = 1
// instance without any (profiles/exact_grid_resource_usage.txt).
constexpr bool fe_grid_instance(int C, int P, bool CHAIN, int NE) {
    if (NE == 1) return true;
    if (NE == 2) return C <= 8;
    return NE == 4 && C <= 4;
}

// Ring depth: the parent's (nb_for(C, P, false)); no part of the arithmetic.
constexpr int fe_grid_nb(int C, int P, bool CHAIN, int NE) { return nb_for(C, P, false); }

template <int NE>
struct FeGrid {
    template <int C, int P, bool CH>
    static hipError_t launch(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
        if constexpr (fe_grid_instance(C, P, CH, NE)) {
            const int bw = ocx_block_waves(L->G);
            hipLaunchKernelGGL(
                (ocx_ftrl_exact_grid_kernel<C, P, CH, fe_grid_nb(C, P, CH, NE), NE>),
                ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
    template <int C, int P, bool CH>
    static hipError_t comp(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
        if constexpr (fe_grid_instance(C, P, CH, NE)) {
            const int64_t n = L->G * a.K;
            const int bw = ocx_block_waves(n);
            hipLaunchKernelGGL(
                (ocx_ftrl_exact_grid_comp_kernel<C, P, CH, nb_for(C, P, false), NE>),
                ocx_grid(n, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
};

template <int C, int P, bool CH>
hipError_t launch_feg1_cp(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
    return FeGrid<1>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_feg2_cp(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
    return FeGrid<2>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_feg4_cp(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
    return FeGrid<4>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_fegc1_cp(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
    return FeGrid<1>::comp<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_fegc2_cp(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
    return FeGrid<2>::comp<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_fegc4_cp(const ocx_layout* L, const FeGridArgs& a, hipStream_t st) {
    return FeGrid<4>::comp<C, P, CH>(L, a, st);
}

hipError_t launch_fe_grid(const ocx_layout* L, const FeGridArgs& a, int NE, hipStream_t st) {
    if (NE == 1) { OCX_DISPATCH(launch_feg1_cp, L, a, st) }
    if (NE == 2) { OCX_DISPATCH(launch_feg2_cp, L, a, st) }
    OCX_DISPATCH(launch_feg4_cp, L, a, st)
}

hipError_t launch_fe_grid_comp(const ocx_layout* L, const FeGridArgs& a, int NE, hipStream_t st) {
    if (NE == 1) { OCX_DISPATCH(launch_fegc1_cp, L, a, st) }
    if (NE == 2) { OCX_DISPATCH(launch_fegc2_cp, L, a, st) }
    OCX_DISPATCH(launch_fegc4_cp, L, a, st)
}

}  // namespace

bool ocx_ftrl_exact_grid_instance(const ocx_layout* L, int group) {
    return (group == 1 || group == 2 || group == 4) &&
           fe_grid_instance(L->C, L->P, L->chain != 0, group);
}

// Columns per pass the dispatcher takes: the largest instance of the layout.  Measured against
// the M single-column calls in every class of sums x coordinates per lane that has one (DESIGN.md
// §3.18, profiles/exact_grid_ab.jsonl), it was the fastest in each, so no class falls back to 1.
int ocx_ftrl_exact_grid_best_group(const ocx_layout* L) {
    return ocx_ftrl_exact_grid_instance(L, 4) ? 4 : (ocx_ftrl_exact_grid_instance(L, 2) ? 2 : 1);
}

int64_t ocx_ftrl_exact_grid_ws_bytes(const ocx_layout* L, int64_t K, int64_t ne, int with_comp_f) {
    return L->G * K * 64 * (8 * (int64_t)L->C * (1 + (with_comp_f ? ne : 0)) + 4);
}

hipError_t ocx_launch_ftrl_exact_grid(const ocx_layout* L, const double* zt, const double* yt,
                                      const double* etas, int64_t M, const int64_t* ck, int64_t K,
                                      double* cum_r, double* cum_e, double* comp_e, double* comp_f,
                                      double* cmp_out, int* regime, int* closed_out, int onepass,
                                      int norm, int group, void* ws, hipStream_t st) {
    if (L->G == 0 || M <= 0 || K <= 0) return hipSuccess;
    if (!ocx_ftrl_exact_grid_instance(L, group)) return hipErrorInvalidValue;
    FeGridArgs a{};
    a.zt = zt;
    a.yt = yt;
    a.B = L->B;
    a.T = L->T;
    a.d = L->d;
    a.G = L->G;
    a.M = M;
    a.ck = ck;
    a.K = K;
    a.cum_r = cum_r;
    a.comp_f = comp_f;
    a.cum_e = cum_e;
    a.comp_e = comp_e;
    a.cmp_out = cmp_out;
    a.regime = regime;
    a.closed_out = closed_out;
    a.onepass = onepass;
    a.norm = norm;
    const int64_t slots = L->G * K * 64;
    for (int64_t m0 = 0; m0 < M; m0 += group) {
        const int ne = (int)(M - m0 < group ? M - m0 : group);
        int NE = ne <= 1 ? 1 : (ne <= 2 ? 2 : 4);  // the smallest instance that holds them
        while (!ocx_ftrl_exact_grid_instance(L, NE)) NE *= 2;  // (`group` is one)
        a.m0 = m0;
        a.ne = ne;
        for (int m = 0; m < kMaxNE; ++m) a.eta[m] = etas[m0 + (m < ne ? m : ne - 1)];
        // this launch's workspace, the three arrays packed for ne (a launch of fewer columns
        // than the first uses a prefix of the same memory)
        a.ws_te = static_cast<double*>(ws);
        a.ws_tr = comp_f != nullptr ? a.ws_te + slots * L->C : nullptr;
        a.ws_need =
            reinterpret_cast<int*>(a.ws_te + slots * L->C * (1 + (comp_f != nullptr ? ne : 0)));
        hipError_t e = launch_fe_grid(L, a, NE, st);
        if (e != hipSuccess) return e;
        e = launch_fe_grid_comp(L, a, NE, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
