// ocx_smart_curve.hip — SMART regret curves: K (horizon, threshold) pairs per read of z.
//
// SMART is as online as FTRL and FTL: its run on (z[:t], y[:t]) with threshold th is the
// first t steps of its run on the whole rows.  The FTL leg and the prefix loss of the switch
// test depend on neither the threshold nor the horizon, and FTRL's step size after the switch
// uses the global step (fast_algorithms.py:149), not T.  So a column of the threshold sweep
// (ocx_smart_thresholds.hip; see its header for the arithmetic, the guard band and what the
// columns share) that stops at step t_k and takes its comparator there IS the run truncated
// at t_k.  Column m of a launch is the pair (h[m], th[m]); the threshold sweep is the case in
// which every horizon is T.
//
// The step is ocx_smart_thresholds_kernel's, statement for statement, written out a second
// time: sharing it behind a compile-time parameter changed the sweep kernels' machine code
// (DESIGN.md §3.12).  What is new is around it.
//
// Segments.  A launch serves nt <= NT consecutive pairs of the list, which is sorted by
// horizon, so its horizons h[0] <= … <= h[NT−1] (spare columns of a tail launch on a copy of
// the last) cut the steps 0 … h[NT−1] into at most NT segments.  The kernel runs the sweep's
// pipelined loop over one segment, freezes the columns whose horizon ends it, and goes on
// with the next; it never looks past its last horizon.  The ring is filled again at the start
// of a segment — one load latency per distinct horizon — so the freeze sits between two
// loops, outside the unrolled ring slots: it costs the loop no registers and its code exists
// once.  The horizons travel in the kernel arguments, so the segment bounds and
// live[m] = (column m is not yet frozen in this segment) are scalar and every branch they
// decide is wave-uniform.
//
// The freeze.  After the step h[m] − 1 (for h[m] = 0: before any step) column m freezes: its
// total is total[m] if it has switched and ftl_loss otherwise, as they stand after h[m]
// steps; its comparator is FTL(theta_ftl after h[m] steps), which is xf as it stands; its
// outputs are written.  In later segments it takes no part in the FTRL branch (it neither
// opens it nor commits), in the switch test or in the re-scan: a step re-scans only while
// some column of the launch is both unswitched and before its horizon.
//
// The comparator, in place.  It is formed at the freeze, once per distinct horizon of the
// launch.  Closed form: h/2 − ||theta_ftl|| where the first h steps certify it; `clean` at
// the freeze is exactly that certificate, per (sequence, column), whatever shares the wave or
// the launch.  Streamed, where __ballot(!closed) says some sequence of the wave needs it: rows
// 0 … h−1 with loads of its own, as the re-scan has, in the parent's second-pass order
// (ocx_total_last per row, then ocx_comp_lane_value), so the sum is the parent's bit for bit
// (through the ring, as the parent streams it, the loop nest cost registers: 8 coordinates per
// lane with two columns fell from two waves per SIMD to one).  No workspace and no second
// kernel: the alternative (§3.9's workspace and ocx_curve_comp_kernel) would keep xf per
// (sequence, column) in HBM and add a launch, for a pass that with both closed forms is not
// run at all and in the re-scan mode is O(h·d) beside the re-scan's O(h²·d).
//
// A column's decisions, and with them every bit of its outputs, do not depend on which other
// columns share its launch: what the columns share does not depend on them, and a frozen
// column is only ever left out.
//
// stats[0] += (sequence, step) pairs that re-scanned, stats[1] += (sequence, column) pairs
// that took the closed comparator, per launch.
//
// Instances and ring depths: the sweep's (NT = 1 for every layout, 2 up to 16 coordinates
// per lane, 4 up to 8).
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

struct SmartCurveArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, d, G;
    const double* thresh;  // [B][K]
    int64_t K, k0;         // row stride, first column of this launch
    int nt;                // columns of this launch (<= the instance's NT)
    int64_t h[4];          // their horizons, non-decreasing; h[nt …] = h[nt − 1]
    double eta0;
    double* regret;        // [B][K]
    int64_t* switch_step;  // [B][K], nullable
    int closed_prefix, closed_comp;
    unsigned long long* stats;  // [2], nullable
};

}  // namespace

template <int C, int P, bool CHAIN, int NB, int NT>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_smart_curve_kernel(SmartCurveArgs a) {
    constexpr int S = 64 / P;
    const int lane = threadIdx.x & 63;
    const int64_t g = ocx_wave_id();
    if (g >= a.G) return;
    const int s = lane / P;
    const int c = lane % P;
    const int64_t b = g * S + s;
    const int64_t B = a.B, T = a.T, d = a.d;
    const int closed_prefix = a.closed_prefix;
    const double eta0 = a.eta0;
    const int64_t tstride = 64;  // ocx_d2 per step within a plane
    const ocx_d2* __restrict__ zp =
        reinterpret_cast<const ocx_d2*>(a.zt) + g * T * tstride + lane;
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k): the batch's T, not a horizon
    const double* __restrict__ yp = a.yt + g * T * S + s;

    // shared: theta_ftl, S_t = Σ y_i z_i, and FTL(theta_ftl) as it stands
    double tf[C], sv[C], xf[C];
#pragma unroll
    for (int j = 0; j < C; ++j) tf[j] = sv[j] = xf[j] = 0.0;
    bool regime = true;  // every row so far in the unit ball, every label ±1
    bool clean = true;   // ... and every FTL sub-gradient −y_t/2 (closed comparator)
    double ftl_loss = 0.0;
    unsigned long long rescans = 0;

    // per column
    double th[NT], tr[NT][C], total[NT];
    bool switched[NT];
    int64_t sw[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        const int mm = m < a.nt ? m : a.nt - 1;
        th[m] = (b < B) ? a.thresh[b * a.K + a.k0 + mm] : 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) tr[m][j] = 0.0;
        total[m] = 0.0;
        switched[m] = (b >= B);  // padding sequences never scan
        sw[m] = -1;
    }

    ocx_d2 zb[NB][C / 2];
    double yb[NB];

    int64_t tb = 0;  // the segment is steps [tb, te)
#pragma unroll 1
    for (int sg = 0; sg < NT; ++sg) {
        int64_t te = a.h[0];
        int64_t prev = -1;
#pragma unroll
        for (int m = 1; m < NT; ++m)
            if (sg >= m) {
                prev = te;
                te = a.h[m];
            }
        if (te == prev) continue;  // frozen with the column before
        // a column takes part in this segment's steps if its horizon is not behind them
        bool live[NT];
#pragma unroll
        for (int m = 0; m < NT; ++m) live[m] = a.h[m] >= te;

#pragma unroll
        for (int u = 0; u < NB - 1; ++u)
            if (tb + u < te) {
                ocx_load_tile<C>(zb[u], zp + (tb + u) * tstride, kst);
                yb[u] = yp[(tb + u) * S];
            }

        for (int64_t t0 = tb; t0 < te; t0 += NB) {
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int64_t t = t0 + u;
                if (t < te) {
                    const int64_t tp = t + NB - 1;
                    if (tp < te) {
                        ocx_load_tile<C>(zb[(u + NB - 1) % NB], zp + tp * tstride, kst);
                        yb[(u + NB - 1) % NB] = yp[tp * S];
                    }
                    const double yv = yb[u];
                    // FTL is always run and updated (:140-146)
                    const double pf = ocx_zdot<C, P, CHAIN>(zb[u], xf, lane);
                    const double dfl = pf - yv;
                    const double gfl = ocx_grad(dfl);
#pragma unroll
                    for (int j = 0; j < C; ++j) tf[j] += gfl * ocx_zj(zb[u], j);
                    const double lf = 0.5 * fabs(dfl);
                    ftl_loss += lf;
                    // whole wave active: the certification sums across lanes
                    const bool rowok = ocx_row_in_ball<C, P>(zb[u]) && fabs(yv) == 1.0;
                    regime = regime && rowok;
                    clean = clean && rowok && gfl == -0.5 * yv;
#pragma unroll
                    for (int j = 0; j < C; ++j) sv[j] += yv * ocx_zj(zb[u], j);  // exact: y = ±1
                    ocx_action_ftl<C, P, CHAIN>(tf, xf, lane);                 // s_t (:157)

                    bool anysw = false, anyun = false;
#pragma unroll
                    for (int m = 0; m < NT; ++m) {
                        anysw = anysw || (live[m] && switched[m]);
                        anyun = anyun || (live[m] && !switched[m]);
                    }
                    if (anysw) {
                        // post-switch: FTRL with the column's own theta and the global t
                        // (:148-154); the columns side by side, committed where switched
                        // and live
                        const double sc = -(eta0 / sqrt((double)(t + 1)));
                        double gr[NT], lr[NT];
#pragma unroll
                        for (int m = 0; m < NT; ++m) {
                            double x[C];
                            const double pr =
                                ocx_ftrl_act_dot_sc<C, P, CHAIN>(tr[m], zb[u], sc, x, lane);
                            const double dr = pr - yv;
                            lr[m] = 0.5 * fabs(dr);
                            gr[m] = ocx_grad(dr);
                        }
#pragma unroll
                        for (int m = 0; m < NT; ++m) {
                            if (live[m] && switched[m]) {
                                total[m] += lr[m];
#pragma unroll
                                for (int j = 0; j < C; ++j)
                                    tr[m][j] += gr[m] * ocx_zj(zb[u], j);
                            }
                        }
                    }
                    if (anyun) {
                        // the switch test (:156-160) of every live unswitched column;
                        // total_loss of such a column is ftl_loss (this step's add included)
                        bool und[NT], fire[NT];
                        bool anyund = false;
#pragma unroll
                        for (int m = 0; m < NT; ++m) {
                            fire[m] = false;
                            // s_loss >= 0, so fl(ftl_loss - s_loss) <= ftl_loss < thresh: the
                            // reference's test is false whatever the prefix
                            und[m] = live[m] && !switched[m] &&
                                     !(closed_prefix && ftl_loss < th[m]);
                            anyund = anyund || und[m];
                        }
                        if (closed_prefix && regime && anyund) {
                            double p[C];
#pragma unroll
                            for (int j = 0; j < C; ++j) p[j] = xf[j] * sv[j];
                            const double dot = ocx_total<C, P, CHAIN>(p, lane);
                            const double n1 = (double)(t + 1);
                            const double s_cl = 0.5 * n1 - 0.5 * dot;
                            const double Dl = ftl_loss - s_cl;
                            const double gbase =
                                n1 * (1e-12 + 2.5e-16 * (2.0 * n1 + 2.0 * (double)d + 8.0));
                            anyund = false;
#pragma unroll
                            for (int m = 0; m < NT; ++m) {
                                if (und[m]) {
                                    const double D = Dl - th[m];
                                    // an infinite threshold must not widen the band, and a
                                    // NaN one never fires
                                    const double tha =
                                        __builtin_isfinite(th[m]) ? fabs(th[m]) : 0.0;
                                    const double guard =
                                        gbase + 4e-16 * (fabs(ftl_loss) + n1 + tha);
                                    if (th[m] != th[m]) {
                                        und[m] = false;
                                    } else if (fabs(D) > guard) {
                                        und[m] = false;
                                        fire[m] = D > 0.0;
                                    }
                                }
                                anyund = anyund || und[m];
                            }
                        }
                        if (anyund) {
                            // the reference's prefix re-scan (:157-160, :79-85), once for
                            // every undecided column: s_loss does not depend on the threshold
                            ++rescans;
                            double s_loss = 0.0;
                            for (int64_t i = 0; i <= t; ++i) {
                                ocx_d2 zi[C / 2];
                                ocx_load_tile<C>(zi, zp + i * tstride, kst);
                                const double q = ocx_zdot<C, P, CHAIN>(zi, xf, lane);
                                s_loss += 0.5 * fabs(q - yp[i * S]);
                            }
                            const double Dr = ftl_loss - s_loss;
#pragma unroll
                            for (int m = 0; m < NT; ++m)
                                if (und[m]) fire[m] = Dr >= th[m];
                        }
#pragma unroll
                        for (int m = 0; m < NT; ++m) {
                            if (fire[m]) {
                                switched[m] = true;
                                sw[m] = t;
                                total[m] = ftl_loss;
                            }
                        }
                    }
                }
            }
        }

        // the freeze of the columns whose horizon is te: comparator = FTL(theta_ftl) = xf
        const bool closed = a.closed_comp && (clean || b >= B);
        double comp = 0.0;
        if (__ballot(!closed) != 0) {  // wave-uniform: stream rows 0 … te − 1
            for (int64_t i = 0; i < te; ++i) {
                ocx_d2 zi[C / 2];
                ocx_load_tile<C>(zi, zp + i * tstride, kst);
                double p[C];
#pragma unroll
                for (int j = 0; j < C; ++j) p[j] = ocx_zj(zi, j) * xf[j];
                const double q = ocx_total_last<C, P, CHAIN>(p, lane);
                comp += 0.5 * fabs(q - yp[i * S]);
            }
            comp = ocx_comp_lane_value<P, CHAIN>(comp, lane);
        }
        if (__ballot(closed) != 0) {
            double p[C];
#pragma unroll
            for (int j = 0; j < C; ++j) p[j] = tf[j] * tf[j];
            const double nrm = sqrt(ocx_total<C, P, CHAIN>(p, lane));
            if (closed) comp = 0.5 * (double)te - nrm;
        }
        if (c == 0 && b < B) {
#pragma unroll
            for (int m = 0; m < NT; ++m) {
                if (m < a.nt && a.h[m] == te) {
                    const int64_t o = b * a.K + a.k0 + m;
                    // a column that never switched: total_loss is ftl_loss (:156)
                    a.regret[o] = (sw[m] >= 0 ? total[m] : ftl_loss) - comp;
                    if (a.switch_step) a.switch_step[o] = sw[m];
                    if (a.stats && closed) atomicAdd(&a.stats[1], 1ULL);
                }
            }
        }
        tb = te;
    }
    if (c == 0 && b < B && a.stats && rescans) atomicAdd(&a.stats[0], rescans);
}

namespace {

// the sweep's instance rule and ring depths (thresh_instance, thresh_nb:
// ocx_smart_thresholds.hip)
constexpr bool curve_instance(int C, int NT) {
    return NT == 1 || (NT == 2 && C <= 16) || (NT == 4 && C <= 8);
}

constexpr int curve_nb(int C, int P, bool CHAIN, int NT) {
    const int nb = nb_for(C, P, false);
    if (P == 1 && C >= 32) return 1;
    return (CHAIN && P >= OCX_CHAIN_WIDE_P && NT > 1) ? (nb / NT < 2 ? 2 : nb / NT) : nb;
}

template <int NT>
struct Curve {
    template <int C, int P, bool CH>
    static hipError_t launch(const ocx_layout* L, const SmartCurveArgs& a, hipStream_t st) {
        if constexpr (curve_instance(C, NT)) {
            const int bw = ocx_block_waves(L->G);
            hipLaunchKernelGGL((ocx_smart_curve_kernel<C, P, CH, curve_nb(C, P, CH, NT), NT>),
                               ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
};

template <int C, int P, bool CH>
hipError_t launch_curve1_cp(const ocx_layout* L, const SmartCurveArgs& a, hipStream_t st) {
    return Curve<1>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_curve2_cp(const ocx_layout* L, const SmartCurveArgs& a, hipStream_t st) {
    return Curve<2>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_curve4_cp(const ocx_layout* L, const SmartCurveArgs& a, hipStream_t st) {
    return Curve<4>::launch<C, P, CH>(L, a, st);
}

hipError_t launch_curve(const ocx_layout* L, const SmartCurveArgs& a, int NT, hipStream_t st) {
    if (NT == 1) { OCX_DISPATCH(launch_curve1_cp, L, a, st) }
    if (NT == 2) { OCX_DISPATCH(launch_curve2_cp, L, a, st) }
    OCX_DISPATCH(launch_curve4_cp, L, a, st)
}

}  // namespace

bool ocx_smart_curve_instance(const ocx_layout* L, int group) {
    return (group == 1 || group == 2 || group == 4) && curve_instance(L->C, group);
}

// The dispatcher's group rule.  Measured (profiles/smart_curve_ab.jsonl) with
// both closed forms on ten horizons 100 … 1000 against ten single-threshold calls on resident
// batches of the first t_k rows, in every class of loop form (chained short and long,
// butterfly of 8 lanes or more, butterfly of fewer lanes, one lane) x coordinates per lane:
// every multi-column group ran 0.55-0.69x of the loop, far outside its spread, and the largest
// instantiated group was the fastest or tied, except at 8 coordinates per lane on 8 lanes or
// more (8 x 8 and 16 x 8 butterfly: group 2 0.59x, group 4 0.67x; the 8 x 8 long chain: 0.60x
// and 0.64x).  Above 16 coordinates per lane there is no multi-column instance: one pass per
// pair.
int ocx_smart_curve_best_group(const ocx_layout* L) {
    if (!curve_instance(L->C, 2)) return 1;
    if (!curve_instance(L->C, 4)) return 2;
    return (L->C == 8 && L->P >= 8) ? 2 : 4;
}

hipError_t ocx_launch_smart_curve(const ocx_layout* L, const double* zt, const double* yt,
                                  const int64_t* hz, const double* th, int64_t K, double eta0,
                                  double* reg, int64_t* sw, int closed_prefix, int closed_comp,
                                  unsigned long long* stats, int group, hipStream_t st) {
    if (L->G == 0 || K <= 0) return hipSuccess;
    if (!ocx_smart_curve_instance(L, group)) return hipErrorInvalidValue;
    SmartCurveArgs a{zt,   yt,  L->B, L->T,          L->d,        L->G, th, K, /*k0*/ 0,
                     /*nt*/ 0,  {0, 0, 0, 0},        eta0,        reg,  sw, closed_prefix,
                     closed_comp, stats};  // k0, nt, h: per launch
    for (int64_t k0 = 0; k0 < K; k0 += group) {
        const int nt = (int)(K - k0 < group ? K - k0 : group);
        const int NT = nt <= 1 ? 1 : (nt <= 2 ? 2 : 4);  // the smallest instance that holds them
        a.k0 = k0;
        a.nt = nt;
        for (int m = 0; m < 4; ++m) a.h[m] = hz[k0 + (m < nt ? m : nt - 1)];
        const hipError_t e = launch_curve(L, a, NT, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
