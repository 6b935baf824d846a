// ocx_smart_thresholds.hip — SMART (fast_algorithms.py:118-164) in lane-group form, for NT
// switch thresholds per pass over z: the single-threshold calls (ocx_launch_smart_closed) run
// its one-column instance, the threshold sweeps (ocx_launch_smart_thresholds) 1, 2 or 4 columns.
//
// Two modes.  closed_prefix = 0: the reference's re-scan at every pre-switch step.
// closed_prefix = 1: O(T·d) per sequence, as follows.
//
// The closed form of the prefix loss.  The reference's SMART re-scans the whole prefix before
// the switch: at every step t it sums ½|z_i·s_t − y_i| over i = 0..t
// (`_comparator_loss_prefix`, :79-85, called at :158), O(T²·d) per sequence, and compares
// ftl_loss − s_loss with the threshold (:159).  On the reference's own data that prefix loss
// has a closed form.  When every row so far lies in the unit ball (||z_i|| <= 1: the g(T)
// sampler and the random families clip them) and every label is ±1, |z_i·s_t| <= 1 for the
// unit-norm FTL action s_t, so ½|z_i·s_t − y_i| = ½(1 − y_i z_i·s_t) and
//
//     s_loss_t = (t+1)/2 − ½ s_t·S_t,   S_t = Σ_{i<=t} y_i z_i,
//
// one dot product per step with S_t kept beside theta in registers.  The closed form differs
// from the reference's sequential sum only by rounding, so it DECIDES the switch only where
// ftl_loss − s_loss is farther from the threshold than a bound on that rounding (`guard`
// below); inside the band, or once a row leaves the ball or a label is not ±1, the step
// re-scans its prefix exactly as the reference does.  The switch step is therefore the
// reference's (bit-identical decisions in the exact layouts), and the regret — total_loss
// minus the comparator loss, both summed as the reference does — is unchanged.
//
// The guard band (u = 2^-53), four error terms:
//  1. the reference's prefix sum differs from the exact value of Σ ½|z_i·s_t − y_i| by at most
//     (t+1)·u·(t + d/2 + 2) (d-term dot products, t+1 ordered adds of terms <= 1);
//  2. that value differs from the closed form's exact value by at most
//     (t+1)·(5e-13 + (d/2 + 4)·u) (rows certified to ||z||² <= 1 + 1e-12, ||s_t|| <= 1 + a few u);
//  3. the computed closed form differs from its exact value by at most (t+1)·u·(t + d + 1)
//     (S_t's sums, the dot, the final subtraction);
//  4. the decision's own subtractions add 2u·(|ftl_loss| + |s| + |thresh|).
// The band is about twice their sum.  An infinite threshold must not widen it (+inf: never
// fires, D = −inf; −inf: fires at once, D = +inf), and a NaN one never fires (`>= NaN` is
// false, :159): both are decided in the band test, not by O(t) re-scans.
//
// The comparator.  The final comparator FTL(theta_ftl) (:162-163) is streamed as the
// reference does, or — closed_comp, not in the bit-exact APIs — taken in closed form
// T/2 − ||theta_ftl|| where every FTL sub-gradient was −y_t/2 (then theta_ftl = −½ S_T; see
// ocx_alg_kernel's onepass comparator), which makes the whole kernel one HBM pass.
//
// What the columns share.  SMART's only parameter is the threshold at which it leaves FTL for
// FTRL, and almost all of `_simulate_SMART_like_core` does not depend on it: the FTL leg
// (theta_ftl, its action, ftl_loss, :140-146), the prefix loss s_loss of the switch test
// (:157-159) and the final comparator.  So there is one copy per sequence of tf, xf, sv,
// ftl_loss, regime, clean, the z / y ring, and the comparator.  What depends on the threshold
// is the step at which ftl_loss − s_loss >= thresh first holds, the FTRL state grown from that
// step on, and total_loss — which before the switch is ftl_loss bit for bit (the same
// additions from 0).
//
// Per column m: switched[m], sw[m], tr[m][C] and total[m].  An unswitched column keeps no
// total of its own: it is ftl_loss, copied at the switch step after that step's add (the
// reference adds the step's FTL loss to total_loss before it tests, :156).  After the switch
// the column takes the FTRL step with its own theta and the global t (:148-154).  The FTRL
// steps of the columns of a sequence run side by side under one branch (some column of the
// sequence has switched) and are committed per column, so that the NT independent chains
// interleave; a column that has not switched runs on theta = 0 and commits nothing.
//
// The switch test runs while some column of the sequence is unswitched.  The shortcut
// ftl_loss < th_m is per column; the closed form s_cl and ftl_loss − s_cl are formed once and
// D_m = (ftl_loss − s_cl) − th_m is taken left to right; the guard takes that column's
// |th_m|.  If any column is left undecided the prefix is re-scanned ONCE and every
// still-undecided column of that step is decided by the reference's
// ftl_loss − s_loss >= th_m: s_loss does not depend on the threshold.  A column's decisions,
// and with them its switch step and every bit of its regret, do not depend on which other
// columns share its pass.
//
// Cross-lane rules: the row certification and the comparator ballots see the whole wave; the
// re-scan and the FTRL branch are uniform per lane group (they depend on the sequence's state
// only).  Padding sequences (b >= B) start with every column switched and read no threshold.
//
// Thresholds are a device array [B][M] (per-sequence thresholds; M = 1 for the
// single-threshold calls); outputs regret [B][M] and switch_step [B][M], this launch's columns
// m0 … m0 + nt − 1.  A launch may hold fewer columns than its instance (nt < NT: 3 of 4): the
// spare column runs on a copy of the last threshold and writes nothing.  stats[0] counts
// (sequence, step) pairs that re-scanned — once per step however many columns needed it —
// and stats[1] the sequences that took the closed comparator, per launch.
//
// Instances: NT = 1 for every layout; NT = 2 up to 16 coordinates per lane; NT = 4 up to 8.
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

struct ThreshArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, d, G;
    const double* thresh;  // [B][M]
    int64_t M, m0;         // row stride, first column of this launch
    int nt;                // columns of this launch (<= the instance's NT)
    double eta0;
    double* regret;        // [B][M]
    int64_t* switch_step;  // [B][M], nullable
    int closed_prefix, closed_comp;
    unsigned long long* stats;  // [2], nullable
};

}  // namespace

template <int C, int P, bool CHAIN, int NB, int NT>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_smart_thresholds_kernel(ThreshArgs a) {
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
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k)
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
        th[m] = (b < B) ? a.thresh[b * a.M + a.m0 + mm] : 0.0;
#pragma unroll
        for (int j = 0; j < C; ++j) tr[m][j] = 0.0;
        total[m] = 0.0;
        switched[m] = (b >= B);  // padding sequences never scan
        sw[m] = -1;
    }

    ocx_d2 zb[NB][C / 2];
    double yb[NB];
#pragma unroll
    for (int u = 0; u < NB - 1; ++u)
        if (u < T) {
            ocx_load_tile<C>(zb[u], zp + u * tstride, kst);
            yb[u] = yp[u * S];
        }

    for (int64_t t0 = 0; t0 < T; t0 += NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int64_t t = t0 + u;
            if (t < T) {
                const int64_t tp = t + NB - 1;
                if (tp < T) {
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
                    anysw = anysw || switched[m];
                    anyun = anyun || !switched[m];
                }
                if (anysw) {
                    // post-switch: FTRL with the column's own theta and the global t
                    // (:148-154); the columns side by side, committed where switched
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
                        if (switched[m]) {
                            total[m] += lr[m];
#pragma unroll
                            for (int j = 0; j < C; ++j) tr[m][j] += gr[m] * ocx_zj(zb[u], j);
                        }
                    }
                }
                if (anyun) {
                    // the switch test (:156-160) of every unswitched column; total_loss of
                    // such a column is ftl_loss (this step's add included)
                    bool und[NT], fire[NT];
                    bool anyund = false;
#pragma unroll
                    for (int m = 0; m < NT; ++m) {
                        fire[m] = false;
                        // s_loss >= 0, so fl(ftl_loss - s_loss) <= ftl_loss < thresh: the
                        // reference's test is false whatever the prefix (any thresh, +inf too)
                        und[m] = !switched[m] && !(closed_prefix && ftl_loss < th[m]);
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
                                // an infinite threshold must not widen the band, and a NaN
                                // one never fires (header, the guard band)
                                const double tha = __builtin_isfinite(th[m]) ? fabs(th[m]) : 0.0;
                                const double guard = gbase + 4e-16 * (fabs(ftl_loss) + n1 + tha);
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
                        // the reference's prefix re-scan (:157-160, :79-85), once for every
                        // undecided column: s_loss does not depend on the threshold
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

    // final comparator = FTL(theta_ftl) (:162-163) = xf
    const bool closed = a.closed_comp && (clean || b >= B);
    double comp = 0.0;
    if (__ballot(!closed) != 0) {  // wave-uniform: stream the second pass
#pragma unroll
        for (int u = 0; u < NB - 1; ++u)
            if (u < T) {
                ocx_load_tile<C>(zb[u], zp + u * tstride, kst);
                yb[u] = yp[u * S];
            }
        for (int64_t t0 = 0; t0 < T; t0 += NB) {
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int64_t t = t0 + u;
                if (t < T) {
                    const int64_t tp = t + NB - 1;
                    if (tp < T) {
                        ocx_load_tile<C>(zb[(u + NB - 1) % NB], zp + tp * tstride, kst);
                        yb[(u + NB - 1) % NB] = yp[tp * S];
                    }
                    double p[C];
#pragma unroll
                    for (int j = 0; j < C; ++j) p[j] = ocx_zj(zb[u], j) * xf[j];
                    const double q = ocx_total_last<C, P, CHAIN>(p, lane);
                    comp += 0.5 * fabs(q - yb[u]);
                }
            }
        }
        comp = ocx_comp_lane_value<P, CHAIN>(comp, lane);
    }
    if (__ballot(closed) != 0) {
        double p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = tf[j] * tf[j];
        const double nrm = sqrt(ocx_total<C, P, CHAIN>(p, lane));
        if (closed) comp = 0.5 * (double)T - nrm;
    }
    if (c == 0 && b < B) {
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            if (m < a.nt) {
                const int64_t o = b * a.M + a.m0 + m;
                // a column that never switched: total_loss is ftl_loss (:156)
                a.regret[o] = (sw[m] >= 0 ? total[m] : ftl_loss) - comp;
                if (a.switch_step) a.switch_step[o] = sw[m];
            }
        }
        if (a.stats) {
            if (rescans) atomicAdd(&a.stats[0], rescans);
            if (closed) atomicAdd(&a.stats[1], 1ULL);
        }
    }
}

namespace {

constexpr bool thresh_instance(int C, int NT) {
    return NT == 1 || (NT == 2 && C <= 16) || (NT == 4 && C <= 8);
}

// Ring depth: nb_for's (the FTRL/FTL kernels'), except for the long exact chains with several
// columns, as in the step-size sweep (etas_nb, ocx_alg_etas.hip): NT copies of the chain code
// in each of nb_for's ring slots pass the compiler's unroll budget, and the ring then stays a
// dynamically indexed array in scratch where one column has none (8 x 16 chained, four
// columns: 272 B per lane).  One lane with 32 coordinates or more (its state vectors alone
// pass the register file, every instance spills) loads each row where it is used, a ring of
// one: at nb_for's two the one-column instance spilled 512 to 2832 B per lane, at one it
// spills 0 to 2036.  The ring depth is no part of the arithmetic.
constexpr int thresh_nb(int C, int P, bool CHAIN, int NT) {
    const int nb = nb_for(C, P, false);
    if (P == 1 && C >= 32) return 1;
    return (CHAIN && P >= OCX_CHAIN_WIDE_P && NT > 1) ? (nb / NT < 2 ? 2 : nb / NT) : nb;
}

template <int NT>
struct Thresholds {
    template <int C, int P, bool CH>
    static hipError_t launch(const ocx_layout* L, const ThreshArgs& a, hipStream_t st) {
        if constexpr (thresh_instance(C, NT)) {
            const int bw = ocx_block_waves(L->G);
            hipLaunchKernelGGL(
                (ocx_smart_thresholds_kernel<C, P, CH, thresh_nb(C, P, CH, NT), NT>),
                ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
};

template <int C, int P, bool CH>
hipError_t launch_thresh1_cp(const ocx_layout* L, const ThreshArgs& a, hipStream_t st) {
    return Thresholds<1>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_thresh2_cp(const ocx_layout* L, const ThreshArgs& a, hipStream_t st) {
    return Thresholds<2>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_thresh4_cp(const ocx_layout* L, const ThreshArgs& a, hipStream_t st) {
    return Thresholds<4>::launch<C, P, CH>(L, a, st);
}

hipError_t launch_thresh(const ocx_layout* L, const ThreshArgs& a, int NT, hipStream_t st) {
    if (NT == 1) { OCX_DISPATCH(launch_thresh1_cp, L, a, st) }
    if (NT == 2) { OCX_DISPATCH(launch_thresh2_cp, L, a, st) }
    OCX_DISPATCH(launch_thresh4_cp, L, a, st)
}

}  // namespace

bool ocx_thresholds_instance(const ocx_layout* L, int group) {
    return (group == 1 || group == 2 || group == 4) && thresh_instance(L->C, group);
}

// The dispatcher's group rule.  Measured (profiles/thresholds_ab.jsonl) with
// both closed forms against M single-threshold calls (then a kernel of their own) on the same
// resident data, in every class of loop form (chained short and long, butterfly of 8 lanes or
// more, butterfly of fewer lanes, one lane) x coordinates per lane: the largest instantiated
// group was the fastest (0.55-0.61x of the loop at M = 4 up to 8 coordinates per lane,
// 0.66-0.72x at 12 and 16, far outside its spread) except in butterfly layouts of 8 lanes or
// more at 8 coordinates per lane (8 x 8, 16 x 8), where group 2 ran 0.65x and group 4 0.69x
// (0.68x against 0.80x at M = 7).  Above 16 coordinates per lane there is no multi-column
// instance: one pass per threshold.
int ocx_thresholds_best_group(const ocx_layout* L) {
    if (!thresh_instance(L->C, 2)) return 1;
    if (!thresh_instance(L->C, 4)) return 2;
    return (L->C == 8 && !L->chain && L->P >= 8) ? 2 : 4;
}

// One threshold per sequence: th, reg, sw [B] read as [B][1], one launch of the one-column
// instance.
hipError_t ocx_launch_smart_closed(const ocx_layout* L, const double* zt, const double* yt,
                                   const double* th, double eta0, double* reg, int64_t* sw,
                                   int closed_prefix, int closed_comp, unsigned long long* stats,
                                   hipStream_t st) {
    if (L->G == 0) return hipSuccess;
    const ThreshArgs a{zt, yt, L->B, L->T, L->d, L->G, th, /*M*/ 1, /*m0*/ 0, /*nt*/ 1,
                       eta0, reg, sw, closed_prefix, closed_comp, stats};
    OCX_DISPATCH(launch_thresh1_cp, L, a, st)
}

hipError_t ocx_launch_smart_thresholds(const ocx_layout* L, const double* zt, const double* yt,
                                       const double* th, int64_t M, double eta0, double* reg,
                                       int64_t* sw, int closed_prefix, int closed_comp,
                                       unsigned long long* stats, int group, hipStream_t st) {
    if (L->G == 0 || M <= 0) return hipSuccess;
    if (!ocx_thresholds_instance(L, group)) return hipErrorInvalidValue;
    ThreshArgs a{zt, yt, L->B, L->T, L->d, L->G, th, M, /*m0*/ 0, /*nt*/ 0,
                 eta0, reg, sw, closed_prefix, closed_comp, stats};  // m0, nt: per launch
    for (int64_t m0 = 0; m0 < M; m0 += group) {
        const int nt = (int)(M - m0 < group ? M - m0 : group);
        const int NT = nt <= 1 ? 1 : (nt <= 2 ? 2 : 4);  // the smallest instance that holds them
        a.m0 = m0;
        a.nt = nt;
        const hipError_t e = launch_thresh(L, a, NT, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
