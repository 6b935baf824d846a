// ocx_alg_etas.hip — step-size sweeps: FTRL (fast_algorithms.py:88-115) for NE values of
// eta0 in one pass over z.
//
// FTRL's per-step state per sequence is small — θ, a few lane partials, the loss and the
// certificate bit — and the rows it reads do not depend on the step size.  The kernels here
// hold that state NE times (NE = 1, 2, 4) and load every z_t / y_t row once per step for all
// of them.  What does not depend on η is formed once per step: the row-in-ball sum of the
// certificate, z_t·z_{t-1} and z_{t-1}·z_{t-1} of the pipelined form, the √(t+1) of the scale
// table.  Everything else is per η: θ, the lane partials A, U and V, g_{t-1}, cum, clean and the
// scale −η/√(t+1).  The columns do NOT share a trajectory: where a row lies outside the unit
// ball |q| can exceed 1, the sub-gradient's sign then depends on η, and θ with it.
//
// Two loop kernels, the multi-η forms of ocx_alg_kernel (ocx_sim.hip) and of the pipelined
// butterfly kernel (ocx_alg_pipe.hip), dispatched by ocx_launch_alg's rule.  Each column's
// arithmetic is that of the kernel it is derived from, operation for operation (the same
// device functions in the plain form; the same fma placement, 64-step U refresh and rescale
// test in the pipelined form), so column m carries the bits of a run of those kernels with
// eta0 = etas[m].  (Their loops stay written out: as calls to the pieces of ocx_alg_step.h two
// measured cases ran 0.5-1.1 % slower)  The pipelined form's rescale-test
// shortcut is decided per column (a ballot of that column's test): both of its branches give
// the same bits, see ocx_alg_pipe.hip.
//
// Comparator: the loss of FTL(θ_T^m), per column.  With the closed form requested it is
// T/2 − ||θ_T^m|| where column m's certificate holds — the row check is shared, the
// sub-gradient check is per column, so the certificate is per (sequence, η).  Every other pair
// gets the streamed second pass, which reads z once per launch (not once per column) and sums
// in the parents' order (ocx_total_last per row, step by step; ocx_comp_pass2 pairs the same
// additions).  A column none of whose pairs in the wave needs it is skipped (wave-uniform), and
// a certified pair keeps the closed form whatever shares its wave or its launch.
//
// The step sizes travel in the kernel arguments (read on the host at call time): no device
// allocation, no synchronisation, capture-safe.  Outputs are [B][M], this launch's columns
// m0 … m0 + ne − 1; a launch may hold fewer columns than its instance (ne < NE: 3 of 4), the
// spare column runs on a copy of the last step size and writes nothing.  NE = 1 is the
// single-η form with strided outputs: the group-1 path of every layout.
//
// Instances: NE = 1 for every layout; NE = 2 up to 16 coordinates per lane; NE = 4 up to 8.
#include "ocx_alg_pipe.h"
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

constexpr int kMaxNE = 4;

struct EtasArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, G;
    double eta[kMaxNE];
    int ne;          // columns of this launch (<= the instance's NE)
    int64_t M, m0;   // output row stride, first column
    double* regret;  // [B][M], each nullable
    double* cum_out;
    double* comp_out;
    int* closed_out;
    int onepass;
};

// Comparator and outputs of both loop forms, th = θ_T per column.  Whole wave active.  `load`
// and the ring (zb, yb) are the loop's own, for the streamed pass.
template <int C, int P, bool CHAIN, int NB, int NE, bool LATE, class IT, class Load>
__device__ __forceinline__ void etas_finish(const EtasArgs& a, double (&th)[NE][C],
                                            const double (&cum)[NE], const bool (&clean)[NE],
                                            ocx_d2 (&zb)[NB][C / 2], double (&yb)[NB],
                                            Load&& load, bool live, int64_t b, int c, int lane) {
    bool closed[NE], need[NE];
    bool any = false;
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        closed[m] = a.onepass && (clean[m] || !live);
        need[m] = m < a.ne && __ballot(!closed[m]) != 0;  // wave-uniform
        any = any || need[m];
    }
    // ---- closed form where certified (ocx_alg_kernel onepass); formed before the streamed
    // pass, which then needs x* only and not θ_T (the order is no part of the arithmetic)
    double cf[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) {
        cf[m] = 0.0;
        if (__ballot(closed[m]) != 0) {  // wave-uniform: the sum below crosses lanes
            double p[C];
#pragma unroll
            for (int j = 0; j < C; ++j) p[j] = th[m][j] * th[m][j];
            const double nrm = sqrt(ocx_total<C, P, CHAIN>(p, lane));
            cf[m] = 0.5 * (double)a.T - nrm;
        }
    }
    double comp[NE];
#pragma unroll
    for (int m = 0; m < NE; ++m) comp[m] = 0.0;
    // ---- streamed pass (fast_algorithms.py:69-76, :113-114) for the columns that need it
    if (any) {
        double xs[NE][C];
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            if (need[m]) {
                ocx_action_ftl<C, P, CHAIN>(th[m], xs[m], lane);
            } else {
#pragma unroll
                for (int j = 0; j < C; ++j) xs[m][j] = 0.0;
            }
        }
        ocx_ring_loop<NB, LATE, IT>(a.T, load, [&](int u, int64_t) {
#pragma unroll
            for (int m = 0; m < NE; ++m) {
                if (need[m]) {
                    double p[C];
#pragma unroll
                    for (int j = 0; j < C; ++j) p[j] = ocx_zj(zb[u], j) * xs[m][j];
                    const double q = ocx_total_last<C, P, CHAIN>(p, lane);
                    comp[m] += 0.5 * fabs(q - yb[u]);
                }
            }
        });
#pragma unroll
        for (int m = 0; m < NE; ++m)
            if (need[m]) comp[m] = ocx_comp_lane_value<P, CHAIN>(comp[m], lane);
    }
#pragma unroll
    for (int m = 0; m < NE; ++m)
        if (closed[m]) comp[m] = cf[m];
    if (c == 0 && live) {
#pragma unroll
        for (int m = 0; m < NE; ++m) {
            if (m < a.ne) {
                const int64_t o = b * a.M + a.m0 + m;
                if (a.regret) a.regret[o] = cum[m] - comp[m];
                if (a.cum_out) a.cum_out[o] = cum[m];
                if (a.comp_out) a.comp_out[o] = comp[m];
                if (a.closed_out) a.closed_out[o] = closed[m] ? 1 : 0;
            }
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Multi-η form of ocx_alg_kernel (algo 0, no caller comparator): every layout the pipelined
// form does not take, the chained exact layouts included.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB, int NE>
__global__ __launch_bounds__(OCX_BLOCK, 1) void ocx_alg_etas_kernel(EtasArgs a) {
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

    // ocx_ftrl_scale's table, the √ shared: −(η/√(t+lane)) of 64 consecutive steps per column
    double scv[NE];
    int64_t base = INT64_MIN / 2;
    ocx_ring_loop<NB>(T, load, [&](int u, int64_t t) {
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
    etas_finish<C, P, CHAIN, NB, NE, false, int64_t>(a, th, cum, clean, zb, yb, load, live, b, c,
                                                     lane);
}

// ---------------------------------------------------------------------------
// Multi-η form of the pipelined butterfly kernel (ocx_alg_pipe.hip, whole runs, FTRL): the
// step is alg_pipe_body's, see there for the lagging state and the lane partials.  Bz and W
// are products of rows only: one copy.
// ---------------------------------------------------------------------------
template <int C, int P, int NB, bool RT, int NE>
__global__ __launch_bounds__(OCX_BLOCK, 1) void ocx_alg_pipe_etas_kernel(EtasArgs a) {
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
    etas_finish<C, P, false, NB, NE, false, IT>(a, th, cum, clean, zb, yb, load, live, b, c, lane);
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
namespace {

constexpr bool etas_instance(int C, int NE) {
    return NE == 1 || (NE == 2 && C <= 16) || (NE == 4 && C <= 8);
}

// Ring depth of the plain form: the parent's, except for the long exact chains with several
// columns.  Their step is NE chained sums long, so the same HBM latency hides behind
// 1/NE as many steps in flight, and NE copies of the chain code in each of the parent's ring
// slots pass the compiler's unroll budget: the ring then stays a dynamically indexed array in
// scratch (528 B per lane at 8 x 8 coordinates) where the parent has none.  The ring depth is
// no part of the arithmetic.
constexpr int etas_nb(int C, int P, bool CHAIN, int NE) {
    const int nb = nb_for(C, P);
    return (CHAIN && P >= OCX_CHAIN_WIDE_P && NE > 1) ? (nb / NE < 2 ? 2 : nb / NE) : nb;
}

template <int NE>
struct PlainEtas {
    template <int C, int P, bool CH>
    static hipError_t launch(const ocx_layout* L, const EtasArgs& a, hipStream_t st) {
        if constexpr (etas_instance(C, NE)) {
            const int bw = ocx_block_waves(L->G);
            hipLaunchKernelGGL((ocx_alg_etas_kernel<C, P, CH, etas_nb(C, P, CH, NE), NE>),
                               ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
};

template <int C, int P, bool CH>
hipError_t launch_etas1_cp(const ocx_layout* L, const EtasArgs& a, hipStream_t st) {
    return PlainEtas<1>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_etas2_cp(const ocx_layout* L, const EtasArgs& a, hipStream_t st) {
    return PlainEtas<2>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_etas4_cp(const ocx_layout* L, const EtasArgs& a, hipStream_t st) {
    return PlainEtas<4>::launch<C, P, CH>(L, a, st);
}

hipError_t launch_plain_etas(const ocx_layout* L, const EtasArgs& a, int NE, hipStream_t st) {
    if (NE == 1) { OCX_DISPATCH(launch_etas1_cp, L, a, st) }
    if (NE == 2) { OCX_DISPATCH(launch_etas2_cp, L, a, st) }
    OCX_DISPATCH(launch_etas4_cp, L, a, st)
}

template <int C, int P, int NE>
hipError_t launch_pipe_etas_cpn(const ocx_layout* L, const EtasArgs& a, hipStream_t st) {
    if constexpr (etas_instance(C, NE)) {
        const int bw = pipe_block_waves(L->G);
        hipLaunchKernelGGL((ocx_alg_pipe_etas_kernel<C, P, pipe_nb<C>(P), pipe_rt<C, P, 1>(), NE>),
                           ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

hipError_t launch_pipe_etas(const ocx_layout* L, const EtasArgs& a, int NE, hipStream_t st) {
    return ocx_pipe_dispatch(L, [&](auto c, auto p) {
        constexpr int C = decltype(c)::value, P = decltype(p)::value;
        switch (NE) {
            case 1: return launch_pipe_etas_cpn<C, P, 1>(L, a, st);
            case 2: return launch_pipe_etas_cpn<C, P, 2>(L, a, st);
            case 4: return launch_pipe_etas_cpn<C, P, 4>(L, a, st);
            default: return hipErrorInvalidValue;
        }
    });
}

}  // namespace

bool ocx_etas_instance(const ocx_layout* L, int group) {
    return (group == 1 || group == 2 || group == 4) && etas_instance(L->C, group);
}

// The dispatcher's group rule: the largest instantiated group.  Measured (DESIGN.md §3.10,
// profiles/etas_ab.jsonl) against M calls of the existing single-η kernels on the same resident
// data, in every class of loop form (pipelined, plain butterfly or one lane, plain chained) x
// coordinates per lane (up to 8: group 4; 12 and 16: group 2): the largest group was the
// fastest in each, 0.33-0.70x of the loop at M = 4 and far outside its spread.  Above 16
// coordinates per lane there is no multi-η instance: one pass per step size.
int ocx_etas_best_group(const ocx_layout* L) {
    return etas_instance(L->C, 4) ? 4 : (etas_instance(L->C, 2) ? 2 : 1);
}

hipError_t ocx_launch_alg_etas(const ocx_layout* L, const double* zt, const double* yt,
                               const double* etas, int64_t M, double* reg, double* cum,
                               double* comp, int* closed_out, int onepass, int group,
                               hipStream_t st) {
    if (L->G == 0 || M <= 0) return hipSuccess;
    if (!ocx_etas_instance(L, group)) return hipErrorInvalidValue;
    EtasArgs a{};
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
    const bool pipe = ocx_alg_use_pipe(L);
    for (int64_t m0 = 0; m0 < M; m0 += group) {
        const int ne = (int)(M - m0 < group ? M - m0 : group);
        const int NE = ne <= 1 ? 1 : (ne <= 2 ? 2 : 4);  // the smallest instance that holds them
        a.m0 = m0;
        a.ne = ne;
        for (int m = 0; m < kMaxNE; ++m) a.eta[m] = etas[m0 + (m < ne ? m : ne - 1)];
        const hipError_t e = pipe ? launch_pipe_etas(L, a, NE, st) : launch_plain_etas(L, a, NE, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
