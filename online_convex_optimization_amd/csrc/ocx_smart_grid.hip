// ocx_smart_grid.hip — SMART regret grids: M thresholds, each observed at K checkpoint
// horizons, per read of z.
//
// The surface R(threshold, T) that chooses SMART's only free parameter is M fixed thresholds
// observed at K horizons.  As a pair list (ocx_smart_curve.hip) that is M·K columns, and a
// threshold's column at t_k and at t_{k+1} are the same run computed twice: SMART is online
// (that file's header).  Here a column is a threshold alone.  It runs once, to the last
// checkpoint, and is observed at every checkpoint on the way; the FTL leg, the switch test's
// prefix loss and the comparator of a checkpoint exist once for all columns of the pass.
//
// The step is ocx_smart_thresholds_kernel's, statement for statement (see its header for the
// arithmetic, the guard band and what the columns share), written out a third time: shared
// behind a compile-time parameter it changed the sweep kernels' machine code.
//
// Segments.  The K checkpoints cut the steps 0 … t_K into segments; the kernel runs the sweep's
// pipelined loop over one segment, emits, and goes on with the next.  The ring is filled again
// at the start of a segment, so the emission sits between two loops, outside the unrolled ring
// slots, as the curve kernel's freeze does.  The checkpoints are a device array read
// wave-uniformly through curve_next (ocx_curve_ck.h), so K is not bounded by the kernel
// arguments and every branch the bounds decide is scalar.
//
// The emission.  No column freezes.  After step t_k − 1 the comparator of t_k is formed once —
// closed form t_k/2 − ||theta_ftl|| where `clean` certifies the first t_k steps, else rows
// 0 … t_k − 1 streamed in place in the parents' second-pass order where __ballot says some
// sequence of the wave needs it — and every column writes (its own total if it has switched,
// else ftl_loss) − comp and its switch step as they stand.  The FTL leg runs to t_K whatever
// the columns do; a step re-scans only while some column of the launch is unswitched.
//
// Element (b, m, k) is bit for bit the lane-group single call on the rows truncated at t_k: the
// column's state after t_k steps does not depend on what follows, and the emission reads it
// without changing it.  It depends neither on the group size nor on the column's neighbours.
//
// A bad checkpoint list is the caller's error on the device entry and gives meaningless numbers,
// but the kernel stays inside the batch and the outputs and terminates: a checkpoint is clamped
// to [0, T], and a segment that would go backwards is empty.
//
// stats[0] += (sequence, step) pairs that re-scanned, stats[1] += (sequence, column,
// checkpoint) triples that took the closed comparator, per launch.
//
// Instances and ring depths: the sweep's (NT = 1 for every layout, 2 up to 16 coordinates per
// lane, 4 up to 8), less one instance and with three shallower rings (grid_instance, grid_nb).
#include "ocx_curve_ck.h"
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"
#include "ocx_smart_grid.h"

namespace {

struct SmartGridArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, d, G;
    const double* thresh;  // [B][M]
    int64_t M, m0;         // row stride, first column of this launch
    int nt;                // columns of this launch (<= the instance's NT)
    const int64_t* ck;     // [K], device
    int64_t K;
    double eta0;
    double* regret;        // [B][M][K]
    int64_t* switch_step;  // [B][M][K], nullable
    int closed_prefix, closed_comp;
    unsigned long long* stats;  // [2], nullable
};

}  // namespace

template <int C, int P, bool CHAIN, int NB, int NT>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_smart_grid_kernel(SmartGridArgs a) {
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
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k): the batch's T, not a checkpoint
    const double* __restrict__ yp = a.yt + g * T * S + s;

    // shared: theta_ftl, S_t = Σ y_i z_i, and FTL(theta_ftl) as it stands
    double tf[C], sv[C], xf[C];
#pragma unroll
    for (int j = 0; j < C; ++j) tf[j] = sv[j] = xf[j] = 0.0;
    bool regime = true;  // every row so far in the unit ball, every label ±1
    bool clean = true;   // ... and every FTL sub-gradient −y_t/2 (closed comparator)
    double ftl_loss = 0.0;
    unsigned long long rescans = 0, nclosed = 0;

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

    int64_t tb = 0;  // the segment is steps [tb, te)
#pragma unroll 1
    for (int64_t k = 0; k < a.K; ++k) {
        // checkpoint k, wave-uniform; never past the batch (curve_next: [0, T + 1])
        int64_t te = curve_next<int64_t>(a.ck, a.K, T, k);
        te = te > T ? T : te;

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
                                for (int j = 0; j < C; ++j)
                                    tr[m][j] += gr[m] * ocx_zj(zb[u], j);
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
                            // reference's test is false whatever the prefix
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

        // the emission at checkpoint te: comparator = FTL(theta_ftl) = xf, once for all columns
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
                if (m < a.nt) {
                    const int64_t o = (b * a.M + a.m0 + m) * a.K + k;
                    // a column that has not switched: total_loss is ftl_loss (:156)
                    a.regret[o] = (sw[m] >= 0 ? total[m] : ftl_loss) - comp;
                    if (a.switch_step) a.switch_step[o] = sw[m];
                }
            }
            if (closed) nclosed += (unsigned long long)a.nt;
        }
        tb = te > tb ? te : tb;  // a segment that would go backwards is empty
    }
    if (c == 0 && b < B && a.stats) {
        if (rescans) atomicAdd(&a.stats[0], rescans);
        if (nclosed) atomicAdd(&a.stats[1], nclosed);
    }
}

namespace {

// The sweep's instance rule (thresh_instance, ocx_smart_thresholds.hip), less one instance:
// the long chain of 8 coordinates on 32 lanes with four columns sits at the curve kernel's 255
// VGPRs, and the checkpoint walk's few more registers took it from two waves per SIMD to one,
// at the sweep's ring of two (144 B of scratch, as the curve kernel) and at a ring of one (no
// scratch, 254 VGPRs + 4 AGPRs).  It is not compiled: that layout runs two columns per pass
// (profiles/smart_grid_resource_usage.txt).
constexpr bool grid_instance(int C, int P, bool CHAIN, int NT) {
    if (CHAIN && C == 8 && P == 32 && NT == 4) return false;
    return NT == 1 || (NT == 2 && C <= 16) || (NT == 4 && C <= 8);
}

// the sweep's ring depths (thresh_nb, ocx_smart_thresholds.hip) ...
constexpr int sweep_nb(int C, int P, bool CHAIN, int NT) {
    const int nb = nb_for(C, P, false);
    if (P == 1 && C >= 32) return 1;
    return (CHAIN && P >= OCX_CHAIN_WIDE_P && NT > 1) ? (nb / NT < 2 ? 2 : nb / NT) : nb;
}

// ... but for three more four-column instances in the same position (6 coordinates per lane on
// 32 and 64 lanes in the butterfly form, 253 VGPRs in the curve kernel; the long chain of 8
// coordinates on 64 lanes), which keep their two waves per SIMD on half the sweep's ring: 2, 2
// and 1.  The ring depth is no part of the arithmetic.
constexpr int grid_nb(int C, int P, bool CHAIN, int NT) {
    const int nb = sweep_nb(C, P, CHAIN, NT);
    if (NT == 4 && ((!CHAIN && C == 6 && P >= 32) || (CHAIN && C == 8 && P == 64))) return nb / 2;
    return nb;
}

template <int NT>
struct Grid {
    template <int C, int P, bool CH>
    static hipError_t launch(const ocx_layout* L, const SmartGridArgs& a, hipStream_t st) {
        if constexpr (grid_instance(C, P, CH, NT)) {
            const int bw = ocx_block_waves(L->G);
            hipLaunchKernelGGL((ocx_smart_grid_kernel<C, P, CH, grid_nb(C, P, CH, NT), NT>),
                               ocx_grid(L->G, bw), dim3(64 * bw), 0, st, a);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
};

template <int C, int P, bool CH>
hipError_t launch_grid1_cp(const ocx_layout* L, const SmartGridArgs& a, hipStream_t st) {
    return Grid<1>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_grid2_cp(const ocx_layout* L, const SmartGridArgs& a, hipStream_t st) {
    return Grid<2>::launch<C, P, CH>(L, a, st);
}
template <int C, int P, bool CH>
hipError_t launch_grid4_cp(const ocx_layout* L, const SmartGridArgs& a, hipStream_t st) {
    return Grid<4>::launch<C, P, CH>(L, a, st);
}

hipError_t launch_grid(const ocx_layout* L, const SmartGridArgs& a, int NT, hipStream_t st) {
    if (NT == 1) { OCX_DISPATCH(launch_grid1_cp, L, a, st) }
    if (NT == 2) { OCX_DISPATCH(launch_grid2_cp, L, a, st) }
    OCX_DISPATCH(launch_grid4_cp, L, a, st)
}

}  // namespace

bool ocx_smart_grid_instance(const ocx_layout* L, int group) {
    return (group == 1 || group == 2 || group == 4) &&
           grid_instance(L->C, L->P, L->chain != 0, group);
}

// The dispatcher's group rule: see DESIGN.md §3.17 for the records it follows.
int ocx_smart_grid_best_group(const ocx_layout* L) {
    if (!ocx_smart_grid_instance(L, 2)) return 1;
    if (!ocx_smart_grid_instance(L, 4)) return 2;
    return (L->C == 8 && L->P >= 8) ? 2 : 4;
}

hipError_t ocx_launch_smart_grid(const ocx_layout* L, const double* zt, const double* yt,
                                 const double* th, int64_t M, const int64_t* ck, int64_t K,
                                 double eta0, double* reg, int64_t* sw, int closed_prefix,
                                 int closed_comp, unsigned long long* stats, int group,
                                 hipStream_t st) {
    if (L->G == 0 || M <= 0 || K <= 0) return hipSuccess;
    if (!ocx_smart_grid_instance(L, group)) return hipErrorInvalidValue;
    SmartGridArgs a{zt, yt, L->B, L->T, L->d, L->G, th, M, /*m0*/ 0, /*nt*/ 0, ck, K,
                    eta0, reg, sw, closed_prefix, closed_comp, stats};  // m0, nt: per launch
    for (int64_t m0 = 0; m0 < M; m0 += group) {
        const int nt = (int)(M - m0 < group ? M - m0 : group);
        const int NT = nt <= 1 ? 1 : (nt <= 2 ? 2 : 4);  // the smallest instance that holds them
        a.m0 = m0;
        a.nt = nt;
        const hipError_t e = launch_grid(L, a, NT, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
