// ocx_alg_curve_etas.hip — regret grids: FTRL (fast_algorithms.py:88-115) for NE values of
// eta0, each observed at K checkpoint horizons t_1 < … < t_K <= T, in one pass over z.
//
// The product of the step-size sweep (ocx_alg_etas.hip) and the regret curve
// (ocx_alg_curve.hip).  The loops are the sweep's: θ, the lane partials, cum and the
// certificate bit held NE times (NE = 1, 2, 4), every z_t / y_t row loaded once per step for
// all of them, what does not depend on η formed once.  Each column's arithmetic is that of
// the sweep's kernel of the same form, operation for operation (the same device functions in
// the plain form; the same fma placement, 64-step U refresh and per-column rescale-test ballot
// in the pipelined form).  The loops stay written out here as they are there: built from shared
// pieces the sweep's loops measured slower.
//
// Each column is observed the way CurveObserver (ocx_alg_curve.hip) observes the parents: the
// next checkpoint is held in a scalar (the list is read through the constant address space,
// ocx_curve_ck.h) and compared with the step counter once per step.  At the top of step
// t == t_k, once every th[m] holds θ_{t_k}^m (the plain kernel: as the step begins; the
// pipelined kernel: right after the lagging θ of each column is brought up to date), cum[m] and
// clean[m] cover the steps before t_k and the kernels emit, per column,
//   - cum, the loss paid in steps 0 … t_k - 1;
//   - the certificate so far — the row check is shared, the sub-gradient check is per column;
//   - where the closed form is requested and certified, t_k/2 − ||θ_{t_k}^m||, the norm summed
//     afresh from θ (ocx_closed_comp).
// t_k = T is emitted after the loop (the pipelined kernel: after its last θ update).  So
// element (b, m, k) carries the bits of a run of the parents' kernels with eta0 = etas[m] on
// the input truncated at t_k.
//
// A triple (sequence, η, checkpoint) that does not take the closed form owes the streamed
// comparator over its prefix.  The loops leave θ_{t_k}^m, cum and a need word in the caller's
// workspace, and ocx_grid_comp_kernel — one wave per (wave-group, checkpoint) — reads the
// launch's need words, exits if none of its pairs needs the pass, and otherwise streams rows
// 0 … t_k - 1 once for all of the launch's columns that need them, each with
// x* = FTL(θ_{t_k}^m) and summed in the order of the parents' second passes (ocx_comp_stream;
// etas_finish is the same multi-column form).  A certified triple keeps the closed form
// whatever shares its wave, its launch or its group.
//
// Workspace of one launch of ne columns (ocx_grid_ws_bytes sizes it for the largest launch;
// the next group of step sizes reuses it, in stream order), slot = (g·K + k)·ne + m:
//   θ     [G·K·ne][C][64] doubles   word j of lane l at ((slot·C + j)·64 + l): coalesced
//   cum   [G·K·ne][64]    doubles
//   need  [G·K·ne][64]    int32     1: the lane's triple takes the streamed pass
//
// The checkpoint array lives in device memory and its order is the caller's precondition.
// Whatever it holds, every access stays inside the batch, the outputs and the workspace: the
// emission index k runs over [0, K) exactly once, rows are addressed by the step counter, and
// the comparator pass clamps its horizon to [0, T].
//
// The step sizes travel in the kernel arguments.  Outputs are [B][M][K], this launch's
// columns m0 … m0 + ne − 1; a launch may hold fewer columns than its instance (ne < NE), the
// spare column runs on a copy of the last step size and writes nothing.
//
// Instances: NE = 1 for every layout; NE = 2 up to 16 coordinates per lane; NE = 4 up to 8 —
// the step-size sweep's set, less two chained instances (grid_instance below).
#include "ocx_alg_pipe.h"
#include "ocx_alg_step.h"
#include "ocx_curve_ck.h"
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

constexpr int kMaxNE = 4;

struct GridArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, G;
    double eta[kMaxNE];
    int ne;          // columns of this launch (<= the instance's NE)
    int64_t M, m0;   // step sizes of the call, first column of this launch
    double* regret;  // [B][M][K], each nullable
    double* cum_out;
    double* comp_out;
    int* closed_out;
    int onepass;
    const int64_t* ck;  // device [K]
    int64_t K;
    double* ws_theta;
    double* ws_cum;
    int* ws_need;
};

// Emission of checkpoint k at horizon tk for every column of the launch, th[m] = θ_{tk}^m.
// Whole wave active (lane exchanges).
template <int C, int P, bool CHAIN, int NE>
__device__ __forceinline__ void grid_emit(const GridArgs& a, int64_t g, int64_t k, int64_t tk,
                                          const double (&th)[NE][C], const double (&cum)[NE],
                                          const bool (&clean)[NE], bool live, int64_t b, int c,
                                          int lane) {
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        if (m < a.ne) {  // wave-uniform
            const bool closed = a.onepass && (clean[m] || !live);
            double comp = 0.0;
            ocx_closed_comp<C, P, CHAIN>(th[m], closed, tk, comp, lane);
            const int64_t slot = (g * a.K + k) * a.ne + m;
            a.ws_need[slot * 64 + lane] = closed ? 0 : 1;
            a.ws_cum[slot * 64 + lane] = cum[m];
            if (__ballot(!closed) != 0) {  // θ for the streamed pass of the uncertified triples
#pragma unroll
                for (int j = 0; j < C; ++j) a.ws_theta[(slot * C + j) * 64 + lane] = th[m][j];
            }
            if (c == 0 && live) {
                const int64_t o = (b * a.M + a.m0 + m) * a.K + k;
                if (a.cum_out) a.cum_out[o] = cum[m];
                if (a.closed_out) a.closed_out[o] = closed ? 1 : 0;
                if (closed) {  // the others: ocx_grid_comp_kernel
                    if (a.comp_out) a.comp_out[o] = comp;
                    if (a.regret) a.regret[o] = cum[m] - comp;
                }
            }
        }
    }
}

// The per-step observer of both loops (CurveObserver's walk over the checkpoint list): emits
// the checkpoints met at step t, and after the loop t_k = T and whatever an unordered list left
// over.  IT: the loop's step type (the comparison stays on the scalar unit).
template <int C, int P, bool CHAIN, int NE, class IT>
struct GridObserver {
    const GridArgs& a;
    int64_t k;
    IT nxt;
    __device__ __forceinline__ explicit GridObserver(const GridArgs& a_)
        : a(a_), k(0), nxt(curve_next<IT>(a_.ck, a_.K, a_.T, 0)) {}
    __device__ __forceinline__ void step(int64_t t, int64_t g, int64_t b, int c, int lane, bool live,
                                         const double (&th)[NE][C], const double (&cum)[NE],
                                         const bool (&clean)[NE]) {
        while ((IT)t >= nxt) {  // wave-uniform
            grid_emit<C, P, CHAIN, NE>(a, g, k, t, th, cum, clean, live, b, c, lane);
            ++k;
            nxt = curve_next<IT>(a.ck, a.K, a.T, k);
        }
    }
    __device__ __forceinline__ void finish(int64_t g, int64_t b, int c, int lane, bool live,
                                           const double (&th)[NE][C], const double (&cum)[NE],
                                           const bool (&clean)[NE]) {
        while (k < a.K) {
            grid_emit<C, P, CHAIN, NE>(a, g, k, a.T, th, cum, clean, live, b, c, lane);
            ++k;
        }
    }
};

}  // namespace

// ---------------------------------------------------------------------------
// Grid form of ocx_alg_etas_kernel: every layout the pipelined form does not take, the chained
// exact layouts included.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB, int NE>
__global__ __launch_bounds__(OCX_BLOCK, 1) void ocx_alg_grid_kernel(GridArgs a) {
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
    const int64_t tstride = 64;  // ocx_d2 per step within a plane
    const ocx_d2* __restrict__ zp = reinterpret_cast<const ocx_d2*>(a.zt) + g * T * tstride + lane;
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k)
    const double* __restrict__ yp = a.yt + g * T * S + s;

    double th[NE][C];
    double cum[NE];
    bool clean[NE];  // every row in the ball, every sub-gradient −y_t/2 so far
#pragma unroll
    for (int m = 0; m < NE; ++m) {
#pragma unroll
        for (int j = 0; j < C; ++j) th[m][j] = 0.0;
        cum[m] = 0.0;
        clean[m] = true;
    }

    ocx_d2 zb[NB][K2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], zp + tl * tstride, kst);
        yb[slot] = yp[tl * S];
    };

    GridObserver<C, P, CHAIN, NE, int64_t> obs(a);
    // ocx_ftrl_scale's table, the √ shared: −(η/√(t+lane)) of 64 consecutive steps per column
    double scv[NE];
    int64_t base = INT64_MIN / 2;
    ocx_ring_loop<NB>(T, load, [&](int u, int64_t t) {
        obs.step(t, g, b, c, lane, live, th, cum, clean);
        const int64_t t1 = t + 1;
        if (t1 - base >= 64 || t1 < base) {
            base = t1;
            const double r = sqrt((double)(t1 + lane));
#pragma unroll
            for (int m = 0; m < NE; ++m) scv[m] = -(a.eta[m] / r);
        }
        // the certificate's row test, once for every column (whole wave active)
        bool inball = true;
        if (ocx_check_rows(onepass)) inball = ocx_row_in_ball<C, P>(zb[u]);
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            const double sc = ocx_readlane(scv[m], (int)(t1 - base));
            double q;  // :105
            if constexpr (CHAIN && P >= OCX_CHAIN_WIDE_P) {
                double fr;
                q = ocx_ftrl_q_sc<C, P, CHAIN>(th[m], zb[u], sc, fr, lane);
            } else {
                double x[C];
                q = ocx_ftrl_act_dot_sc<C, P, CHAIN>(th[m], zb[u], sc, x, lane);
            }
            const double diff = q - yb[u];  // :106-111
            cum[m] += 0.5 * fabs(diff);
            const double gq = ocx_grad(diff);
            clean[m] = clean[m] & inball;
            clean[m] = clean[m] && fabs(yb[u]) == 1.0 && gq == -0.5 * yb[u];
#pragma unroll
            for (int j = 0; j < C; ++j) th[m][j] += gq * ocx_zj(zb[u], j);  // gq*z is exact
        }
    });
    obs.finish(g, b, c, lane, live, th, cum, clean);
}

// ---------------------------------------------------------------------------
// Grid form of ocx_alg_pipe_etas_kernel (the pipelined butterfly step, see ocx_alg_pipe.hip for
// the lagging state and the lane partials).  Bz and W are products of rows only: one copy.
// ---------------------------------------------------------------------------
template <int C, int P, int NB, bool RT, int NE>
__global__ __launch_bounds__(OCX_BLOCK, 1) void ocx_alg_pipe_grid_kernel(GridArgs a) {
    static_assert(P >= 2 && NB >= 4, "butterfly layouts, a ring holding z_{t-1} .. z_{t+1}");
    using IT = pipe_step_t<C>;
    constexpr int S = 64 / P;
    constexpr int K2 = C / 2;
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)__builtin_amdgcn_readfirstlane((int)ocx_pipe_wave_id(a.G));
    if (g >= a.G) return;
    const int64_t T = a.T;
    const int s = lane / P;
    const int c = lane % P;
    const int64_t b = g * S + s;
    const bool live = b < a.B;
    const int64_t tstride = 64;  // ocx_d2 per step within a plane
    const ocx_d2* __restrict__ zg = reinterpret_cast<const ocx_d2*>(a.zt) + g * T * tstride;
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k)
    const double* __restrict__ yg = a.yt + g * T * S;

    double th[NE][C];  // θ_{t-1} (lagging one update)
    double gp[NE];     // g_{t-1}
    double A[NE], U[NE], V[NE];  // step t's lane partials that depend on θ
    double Bz = 0.0, W = 0.0;    // z_t·z_{t-1}, z_{t-1}·z_{t-1}
    double cum[NE];
    bool clean[NE];
    double scv[NE];  // −η/√(t+1+lane) for the 64 steps from the last multiple of 64
#pragma unroll
    for (int m = 0; m < NE; ++m) {
#pragma unroll
        for (int j = 0; j < C; ++j) th[m][j] = 0.0;
        gp[m] = A[m] = U[m] = V[m] = cum[m] = scv[m] = 0.0;
        clean[m] = true;
    }

    ocx_d2 zb[NB][K2];
    double yb[NB];
#pragma unroll
    for (int k = 0; k < K2; ++k) zb[NB - 1][k] = ocx_d2{0.0, 0.0};
    auto load = [&](int slot, int64_t tl) {
        const ocx_d2* __restrict__ row = zg + tl * tstride;  // uniform
#pragma unroll
        for (int k = 0; k < K2; ++k) {
#if OCX_LOAD_NT
            zb[slot][k] = __builtin_nontemporal_load(row + k * kst + lane);
#else
            zb[slot][k] = row[k * kst + lane];
#endif
        }
        yb[slot] = yg[tl * S + s];
    };

    GridObserver<C, P, false, NE, IT> obs(a);
    ocx_ring_loop<NB, true, IT>(T, load, [&](int u, int64_t t) {
        if ((t & 63) == 0) {
            const double r = sqrt((double)(t + 1 + lane));
#pragma unroll
            for (int m = 0; m < NE; ++m) {
                scv[m] = -(a.eta[m] / r);
                double uu = 0.0;
#pragma unroll
                for (int j = 0; j < C; ++j) uu = __builtin_fma(th[m][j], th[m][j], uu);
                U[m] = uu;
            }
        }
        const ocx_d2* zp1 = zb[(u + NB - 1) % NB];
        const double yv = yb[u];
        double zth[NE], tth[NE], gq[NE];
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            // ---- chain: g_{t-1} → z_t·θ_t, ||θ_t||² → q_t → g_t
            zth[m] = __builtin_fma(gp[m], Bz, A[m]);
            tth[m] = __builtin_fma(gp[m], __builtin_fma(gp[m], W, 2.0 * V[m]), U[m]);
            // θ_t = θ_{t-1} + g_{t-1} z_{t-1} (exact: g is a power of two or 0)
#pragma unroll
            for (int j = 0; j < C; ++j)
                th[m][j] = __builtin_fma(gp[m], ocx_zj(zp1, j), th[m][j]);
        }
        obs.step(t, g, b, c, lane, live, th, cum, clean);  // every th[m] holds θ_t^m
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            const double q_raw = ocx_seq_sum<P>(zth[m]);
            const double n_raw = ocx_seq_sum<P>(tth[m]);
            const double sc = ocx_readlane(scv[m], (int)(t & 63));  // −η/√(t+1)
            const double qa = sc * q_raw;
            double q;
            // the parent's rescale-test shortcut, this column's ballot
            if (RT && __ballot(sc * sc * n_raw >= 1.0 - 1e-12) == 0) {
                q = qa;
            } else {
                const double s_abs = fabs(sc) * sqrt(n_raw > 0.0 ? n_raw : 0.0);
                q = s_abs > 1.0 ? qa * (1.0 / s_abs) : qa;
            }
            const double diff = q - yv;  // :106-111
            cum[m] += 0.5 * fabs(diff);
            gq[m] = ocx_grad(diff);
            clean[m] = clean[m] && fabs(yv) == 1.0 && gq[m] == -0.5 * yv;
        }
        // ---- off the chain: step t+1's lane partials (θ_t is known, g_t is not)
        const ocx_d2* zc = zb[u];
        const ocx_d2* zn = zb[(u + 1) % NB];  // z_{t+1}, in flight since NB-2 steps
        double w = 0.0, bn = 0.0;
        double an[NE];
#pragma unroll
        for (int m = 0; m < NE; ++m) an[m] = 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const double zj = ocx_zj(zc, j);
            w = __builtin_fma(zj, zj, w);
            bn = __builtin_fma(ocx_zj(zn, j), zj, bn);
#pragma unroll
            for (int m = 0; m < NE; ++m) an[m] = __builtin_fma(ocx_zj(zn, j), th[m][j], an[m]);
        }
        if (ocx_check_rows(a.onepass)) {  // row t in the ball: once for every column
            const bool inball = ocx_seq_sum<P>(w) <= 1.0 + 1e-12;
#pragma unroll
            for (int m = 0; m < NE; ++m) clean[m] = clean[m] & inball;
        }
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            V[m] = zth[m];
            U[m] = tth[m];
            A[m] = an[m];
            gp[m] = gq[m];
        }
        W = w;
        Bz = bn;
    });
    // θ_T = θ_{T-1} + g_{T-1} z_{T-1} (the row loaded again: its ring slot is not known at
    // compile time)
    if (T > 0) {
        ocx_d2 zl[K2];
        ocx_load_tile<C>(zl, zg + (T - 1) * tstride + lane, kst);
#pragma unroll
        for (int m = 0; m < NE; ++m) {
#pragma unroll
            for (int j = 0; j < C; ++j) th[m][j] = __builtin_fma(gp[m], ocx_zj(zl, j), th[m][j]);
        }
    }
    obs.finish(g, b, c, lane, live, th, cum, clean);
}

// ---------------------------------------------------------------------------
// The streamed comparator of the launch's uncertified triples: wave w = g·K + k sums
// ½|z_t·x* − y_t| over rows 0 … t_k - 1 of wave-group g once for every column m of the launch
// that needs it, x* = FTL(θ_{t_k}^m) from the workspace, in the order of the parents' second
// passes (ocx_comp_stream per column; etas_finish is the same multi-column form).
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB, int NE>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_grid_comp_kernel(GridArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = ocx_wave_id();
    if (w >= a.G * a.K) return;
    const int64_t g = w / a.K, k = w - g * a.K;
    bool mine[NE], need[NE];
    bool any = false;
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        mine[m] = m < a.ne && a.ws_need[((w * a.ne + m) * 64) + lane] != 0;
        need[m] = __ballot(mine[m]) != 0;  // wave-uniform
        any = any || need[m];
    }
    if (!any) return;  // every triple of this wave is certified
    const int64_t T = a.T;
    int64_t tk = curve_ck(a.ck, k);
    tk = tk < 0 ? 0 : (tk > T ? T : tk);
    const OcxSeq<P> q(a.zt, a.yt, g, a.B, T, a.G);
    double xs[NE][C];
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        if (need[m]) {
            const int64_t slot = w * a.ne + m;
            double th[C];
#pragma unroll
            for (int j = 0; j < C; ++j) th[j] = a.ws_theta[(slot * C + j) * 64 + lane];
            ocx_action_ftl<C, P, CHAIN>(th, xs[m], lane);
        } else {
#pragma unroll
            for (int j = 0; j < C; ++j) xs[m][j] = 0.0;
        }
    }
    ocx_d2 zb[NB][C / 2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], q.zp + tl * 64, q.kst);
        yb[slot] = q.yp[tl * q.S];
    };
    double comp[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) comp[m] = 0.0;
    ocx_ring_loop<NB>(tk, load, [&](int u, int64_t) {
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            if (need[m]) {
                double p[C];
#pragma unroll
                for (int j = 0; j < C; ++j) p[j] = ocx_zj(zb[u], j) * xs[m][j];
                const double qq = ocx_total_last<C, P, CHAIN>(p, lane);
                comp[m] += 0.5 * fabs(qq - yb[u]);
            }
        }
    });
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        if (need[m]) {
            const double cv = ocx_comp_lane_value<P, CHAIN>(comp[m], lane);
            if (mine[m] && q.c == 0 && q.live) {
                const int64_t o = (q.b * a.M + a.m0 + m) * a.K + k;
                if (a.comp_out) a.comp_out[o] = cv;
                if (a.regret) a.regret[o] = a.ws_cum[(w * a.ne + m) * 64 + lane] - cv;
            }
        }
    }
}

// gmax[n] = max(start, max_b r[b][n]) over r [B][N], start +0.0 or (accumulate) what gmax[n]
// holds: ocx_max_kernel's `v > max` scan per column, so a column of negative regrets gives +0.0
// and NaNs are ignored.  One block per column.
__global__ __launch_bounds__(OCX_BLOCK) void ocx_max_cols_kernel(const double* __restrict__ r,
                                                                 int64_t B, int64_t N,
                                                                 double* __restrict__ gmax,
                                                                 int accumulate) {
    __shared__ double sm[OCX_BLOCK];
    const int64_t n = blockIdx.x;
    if (n >= N) return;
    double m = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += OCX_BLOCK) {
        const double v = r[i * N + n];
        if (v > m) m = v;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int w = OCX_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && sm[threadIdx.x + w] > sm[threadIdx.x])
            sm[threadIdx.x] = sm[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double v = sm[0];
        if (accumulate) {
            const double old = gmax[n];
            if (old > v) v = old;
        }
        gmax[n] = v;
    }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
namespace {

// The step-size sweep's set (etas_instance, ocx_alg_etas.hip), less two chained instances at 8
// coordinates per lane — NE = 4 on 32 lanes, NE = 2 on 64 — whose ring stays in scratch
// (144 B per lane) even at the shallowest depth while their step-size twins have none
// (profiles/grid_resource_usage.txt): their groups take the next instance.
constexpr bool grid_instance(int C, int P, bool CHAIN, int NE) {
    if (CHAIN && C == 8 && ((P == 32 && NE == 4) || (P == 64 && NE == 2))) return false;
    return NE == 1 || (NE == 2 && C <= 16) || (NE == 4 && C <= 8);
}

// Ring depth of the plain form and of the comparator: etas_nb's (ocx_alg_etas.hip) — the
// parent's, shallower for the long exact chains with several columns.  With the emission in
// the loop body three more chained instances pass the compiler's unroll budget at that depth
// (the ring then stays a dynamically indexed array in scratch where the step-size twin has
// none): they run the deepest ring that stays in registers.  No part of the arithmetic.
constexpr int grid_nb(int C, int P, bool CHAIN, int NE) {
    const int nb = nb_for(C, P);
    if (CHAIN && P >= OCX_CHAIN_WIDE_P && NE > 1) return nb / NE < 2 ? 2 : nb / NE;
    if (CHAIN && P == 64 && NE == 1 && C == 8) return 3;   // 4: 272 B per lane
    if (CHAIN && P == 64 && NE == 1 && C == 16) return 2;  // 3: 400 B per lane
    if (CHAIN && P == 4 && NE == 4 && C == 8) return 4;    // 8: 528 B per lane
    return nb;
}

template <int NE>
struct PlainGrid {
    template <int C, int P, bool CH>
    static hipError_t launch(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
        if constexpr (grid_instance(C, P, CH, NE)) {
            const int bw = ocx_block_waves(L->G);
            hipLaunchKernelGGL((ocx_alg_grid_kernel<C, P, CH, grid_nb(C, P, CH, NE), NE>),
                               ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
    template <int C, int P, bool CH>
    static hipError_t comp(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
        if constexpr (grid_instance(C, P, CH, NE)) {
            const int64_t n = L->G * a.K;
            const int bw = ocx_block_waves(n);
            hipLaunchKernelGGL((ocx_grid_comp_kernel<C, P, CH, grid_nb(C, P, CH, NE), NE>),
                               ocx_grid(n, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
};

template <int C, int P, bool CH>
hipError_t launch_grid1_cp(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
    return PlainGrid<1>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_grid2_cp(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
    return PlainGrid<2>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_grid4_cp(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
    return PlainGrid<4>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_gcomp1_cp(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
    return PlainGrid<1>::comp<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_gcomp2_cp(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
    return PlainGrid<2>::comp<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_gcomp4_cp(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
    return PlainGrid<4>::comp<C, P, CH>(L, a, st);
}

hipError_t launch_plain_grid(const ocx_layout* L, const GridArgs& a, int NE, hipStream_t st) {
    if (NE == 1) { OCX_DISPATCH(launch_grid1_cp, L, a, st) }
    if (NE == 2) { OCX_DISPATCH(launch_grid2_cp, L, a, st) }
    OCX_DISPATCH(launch_grid4_cp, L, a, st)
}

hipError_t launch_grid_comp(const ocx_layout* L, const GridArgs& a, int NE, hipStream_t st) {
    if (NE == 1) { OCX_DISPATCH(launch_gcomp1_cp, L, a, st) }
    if (NE == 2) { OCX_DISPATCH(launch_gcomp2_cp, L, a, st) }
    OCX_DISPATCH(launch_gcomp4_cp, L, a, st)
}

template <int C, int P, int NE>
hipError_t launch_pipe_grid_cpn(const ocx_layout* L, const GridArgs& a, hipStream_t st) {
    if constexpr (grid_instance(C, P, false, NE)) {
        const int bw = pipe_block_waves(L->G);
        hipLaunchKernelGGL((ocx_alg_pipe_grid_kernel<C, P, pipe_nb<C>(P), pipe_rt<C, P, 1>(), NE>),
                           ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

hipError_t launch_pipe_grid(const ocx_layout* L, const GridArgs& a, int NE, hipStream_t st) {
    return ocx_pipe_dispatch(L, [&](auto c, auto p) {
        constexpr int C = decltype(c)::value, P = decltype(p)::value;
        switch (NE) {
            case 1: return launch_pipe_grid_cpn<C, P, 1>(L, a, st);
            case 2: return launch_pipe_grid_cpn<C, P, 2>(L, a, st);
            case 4: return launch_pipe_grid_cpn<C, P, 4>(L, a, st);
            default: return hipErrorInvalidValue;
        }
    });
}

}  // namespace

bool ocx_grid_instance(const ocx_layout* L, int group) {
    return (group == 1 || group == 2 || group == 4) &&
           grid_instance(L->C, L->P, L->chain != 0, group);
}

// The dispatcher's group rule starts from the step-size sweep's (ocx_etas_best_group): the
// largest instantiated group, 4 up to 8 coordinates per lane, 2 up to 16, 1 above.  Measured
// for the grid itself (profiles/grid_ab.jsonl) in every class of loop form x
// coordinates per lane, the largest group was the fastest in each but one: the pipelined 8-lane
// layout at 4 coordinates per lane (65 536 x 5e3 x 32: group 4 34.67 ms, group 2 30.59 ms; its
// NE = 4 instance runs one wave per SIMD where NE = 2 runs two), which runs group 2.
int ocx_grid_best_group(const ocx_layout* L) {
    if (L->P == 8 && L->C == 4 && ocx_alg_use_pipe(L)) return 2;
    return ocx_grid_instance(L, 4) ? 4 : (ocx_grid_instance(L, 2) ? 2 : 1);
}

int64_t ocx_grid_ws_bytes(const ocx_layout* L, int64_t K, int64_t ne) {
    return L->G * K * ne * 64 * (8 * (int64_t)L->C + 8 + 4);
}

hipError_t ocx_launch_alg_grid(const ocx_layout* L, const double* zt, const double* yt,
                               const double* etas, int64_t M, const int64_t* ck, int64_t K,
                               double* reg, double* cum, double* comp, int* closed_out,
                               int onepass, int group, void* ws, hipStream_t st) {
    if (L->G == 0 || M <= 0 || K <= 0) return hipSuccess;
    if (!ocx_grid_instance(L, group)) return hipErrorInvalidValue;
    GridArgs a{};
    a.zt = zt;
    a.yt = yt;
    a.B = L->B;
    a.T = L->T;
    a.G = L->G;
    a.M = M;
    a.regret = reg;
    a.cum_out = cum;
    a.comp_out = comp;
    a.closed_out = closed_out;
    a.onepass = onepass;
    a.ck = ck;
    a.K = K;
    const bool pipe = ocx_alg_use_pipe(L);
    for (int64_t m0 = 0; m0 < M; m0 += group) {
        const int ne = (int)(M - m0 < group ? M - m0 : group);
        int NE = ne <= 1 ? 1 : (ne <= 2 ? 2 : 4);  // the smallest instance that holds them
        while (!ocx_grid_instance(L, NE)) NE *= 2;   // (`group` is one)
        a.m0 = m0;
        a.ne = ne;
        for (int m = 0; m < kMaxNE; ++m) a.eta[m] = etas[m0 + (m < ne ? m : ne - 1)];
        // this launch's workspace: ne columns per (group, checkpoint), the three arrays packed
        // for ne (a launch of fewer columns than the first uses a prefix of the same memory)
        const int64_t slots = L->G * K * ne * 64;
        a.ws_theta = static_cast<double*>(ws);
        a.ws_cum = a.ws_theta + slots * L->C;
        a.ws_need = reinterpret_cast<int*>(a.ws_cum + slots);
        hipError_t e = pipe ? launch_pipe_grid(L, a, NE, st) : launch_plain_grid(L, a, NE, st);
        if (e != hipSuccess) return e;
        e = launch_grid_comp(L, a, NE, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t ocx_launch_max_cols(const double* r, int64_t B, int64_t N, double* gmax,
                               int accumulate, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(ocx_max_cols_kernel, dim3((unsigned)N), dim3(OCX_BLOCK), 0, st, r, B, N,
                       gmax, accumulate);
    return hipGetLastError();
}
