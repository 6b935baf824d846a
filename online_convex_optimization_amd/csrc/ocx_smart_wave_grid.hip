// ocx_smart_wave_grid.hip — the grid form of ocx_smart_wave_cols_kernel
// (ocx_smart_wave_cols.hip): SMART with one wavefront per sequence for up to NT thresholds per
// prefix re-scan, each observed at K checkpoint horizons.
//
// It is that kernel with no freeze.  A column is a threshold alone: it runs to the last
// checkpoint and is observed at every checkpoint on the way.  What a column owns is
// theta_ftrl (coordinate `lane`), its total loss, its switch step and a flag; theta_ftl,
// ftl_loss, the FTL leg of every step (kSpec steps ahead), one prefix_loss_multi per speculated
// group and one comparator scan per checkpoint exist once per sequence.
//
// The summation pieces are ocx_smart_wave_kernel's.  The ordered adder, the sub-gradient and
// the FTL action are one copy, in ocx_smart_wave.h; prefix_loss, prefix_loss_multi with its
// DMAX = 8 and DMAX = 0 row paths, the tile addressing by readlane, the interleaved column sums
// and the FTRL step of the columns are the column kernel's operation for operation, written out
// a third time here (shared, they change the device assembly: DESIGN.md §3.13).  They add in
// the reference's order whatever the layout, so every element carries the C oracle's bits.
//
// Checkpoints.  They are a device int64 array [K], read wave-uniformly through curve_next
// (ocx_curve_ck.h) and clamped to [0, T].  A speculated group never crosses the next
// checkpoint: K = min(kSpec, t_k − t).  When t reaches t_k the comparator
// prefix_loss(FTL(theta_ftl), t_k) is taken once and every column of the launch is emitted:
// its own total if it has switched, else ftl_loss, minus the comparator, and its switch step
// as it stands.  The spare columns of a tail launch (m >= nt) are never live: they are neither
// tested nor written and do not keep the re-scan alive.  A checkpoint behind t (a bad list:
// the caller's error) is emitted where it stands, from rows inside the batch, and the walk
// goes on: the kernel terminates after at most T steps and K emissions.
//
// stats[0] += (sequence, step) pairs whose switch test ran, once per step however many columns
// needed it, up to the last undecided column's switch or the last checkpoint:
// Σ_b max_m (pre-switch steps of column m, capped at t_K), the lane-group grid's re-scan count.
#include "ocx_curve_ck.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"
#include "ocx_smart_grid.h"
#include "ocx_smart_wave.h"

namespace {

constexpr int kGridBlock = 256;

struct WaveGridArgs {
    const double* zt;
    const double* yt;
    int64_t B, T;
    int d, P, C;
    int64_t G;
    const double* thresh;  // [B][M]
    int64_t M, m0;         // row stride, first column of this launch
    int nt;                // columns of this launch (<= the instance's NT)
    const int64_t* ck;     // [K], device
    int64_t K;
    double eta0;
    double* regret;        // [B][M][K]
    int64_t* switch_step;  // [B][M][K], nullable
    unsigned long long* stats;  // [2], nullable
};

// NT of those sums from 0.0 side by side: out[m] = v[m]_0 + ... + v[m]_{n-1}, each left to
// right, the NT dependent chains interleaved through NT x 64 slots of `buf`.
template <int NT>
__device__ __forceinline__ void ordered_sum_grid_cols(const double (&v)[NT], int n, double* buf,
                                                      int lane, double (&out)[NT]) {
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        buf[m * 64 + lane] = v[m];
        out[m] = 0.0;
    }
    __builtin_amdgcn_wave_barrier();
    int u = 0;
    for (; u + 4 <= n; u += 4) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int m = 0; m < NT; ++m) out[m] += buf[m * 64 + u + w];
    }
    for (; u < n; ++u)
#pragma unroll
        for (int m = 0; m < NT; ++m) out[m] += buf[m * 64 + u];
    __builtin_amdgcn_wave_barrier();
}

}  // namespace

template <int DMAX, int NT>
__global__ __launch_bounds__(kGridBlock) void ocx_smart_wave_grid_kernel(WaveGridArgs a) {
    constexpr int kBuf = kSpec > NT ? kSpec : NT;  // 64-double LDS rows per wave
    __shared__ double bufs[kGridBlock * kBuf];
    const int lane = threadIdx.x & 63;
    double* buf = bufs + (threadIdx.x & ~63) * kBuf;
    const int64_t b = (int64_t)blockIdx.x * (kGridBlock / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const double* __restrict__ zt = a.zt;
    const int64_t T = a.T, G = a.G;
    const int d = a.d, P = a.P, C = a.C, nt = a.nt;
    const double eta0 = a.eta0;
    const int S = 64 / P;
    const int64_t g = b / S;
    const int s = (int)(b - g * S);
    const bool own = lane < d;  // this lane's coordinate j = lane exists
    // tile offset of coordinate `lane` of this sequence at step 0 (+ t·128 for step t)
    int64_t zoff = 0;
    if (own) {
        const int c = lane / C, rr = lane - c * C;
        zoff = ((int64_t)(rr >> 1) * G + g) * T * 128 + (s * P + c) * 2 + (rr & 1);
    }
    const double* __restrict__ yp = a.yt + g * T * S + s;  // y_t = yp[t * S]

    // ½|z_i·sv − y_i| summed over rows i < n in order: lane ℓ forms the terms of rows
    // i0 + ℓ (coordinates read from the lanes that own them), the wave adds them.  With
    // DMAX > 0 (d <= DMAX) the next chunk's rows are loaded while this chunk is summed.
    auto offset_of = [&](int j) -> int64_t {
        return ((int64_t)__builtin_amdgcn_readlane((int)(zoff >> 32), j) << 32) |
               (uint32_t)__builtin_amdgcn_readlane((int)zoff, j);
    };
    auto coord_of = [&](double v, int j) -> double {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j),
                                __builtin_amdgcn_readlane(__double2loint(v), j));
    };
    auto prefix_loss = [&](double sv, int64_t n) -> double {
        double tot = 0.0;
        if constexpr (DMAX > 0) {
            double zc[DMAX], yc = 0.0;
            auto load = [&](int64_t i0, double (&zb)[DMAX], double& yb) {
                const int64_t i = (i0 + lane < n) ? i0 + lane : 0;
#pragma unroll
                for (int j = 0; j < DMAX; ++j) zb[j] = (j < d) ? zt[offset_of(j) + i * 128] : 0.0;
                yb = yp[i * S];
            };
            if (n > 0) load(0, zc, yc);
            for (int64_t i0 = 0; i0 < n; i0 += 64) {
                const int m = (int)((n - i0) < 64 ? (n - i0) : 64);
                double zn[DMAX], yn = 0.0;
                if (i0 + 64 < n) load(i0 + 64, zn, yn);
                double q = 0.0;
#pragma unroll
                for (int j = 0; j < DMAX; ++j)
                    if (j < d) q += zc[j] * coord_of(sv, j);
                const double h = 0.5 * fabs(q - yc);
                tot = ordered_sum(tot, h, m, buf, lane);
#pragma unroll
                for (int j = 0; j < DMAX; ++j) zc[j] = zn[j];
                yc = yn;
            }
        } else {
            for (int64_t i0 = 0; i0 < n; i0 += 64) {
                const int m = (int)((n - i0) < 64 ? (n - i0) : 64);
                const int64_t i = i0 + (lane < m ? lane : 0);
                double q = 0.0;
                for (int j = 0; j < d; ++j) q += zt[offset_of(j) + i * 128] * coord_of(sv, j);
                const double h = 0.5 * fabs(q - yp[i * S]);
                tot = ordered_sum(tot, h, m, buf, lane);
            }
        }
        return tot;
    };
    // The prefix losses of kSpec consecutive steps t..t+K-1 at once: sv[k] = s_{t+k}, rows
    // 0..t+k each.  The chunk's rows are shared; a row beyond t+k contributes +0.0 to
    // chain k, which leaves that sum unchanged.  The K ordered chains interleave.
    auto prefix_loss_multi = [&](const double (&sv)[kSpec], int64_t t, int K,
                                 double (&out)[kSpec]) {
#pragma unroll
        for (int k = 0; k < kSpec; ++k) out[k] = 0.0;
        const int64_t n = t + K;
        auto chunk = [&](int64_t i0, const double* zr, double yr) {
            const int m = (int)((n - i0) < 64 ? (n - i0) : 64);
            const int64_t i = i0 + lane;
#pragma unroll
            for (int k = 0; k < kSpec; ++k) {
                double q = 0.0;
                if constexpr (DMAX > 0) {
#pragma unroll
                    for (int j = 0; j < DMAX; ++j)
                        if (j < d) q += zr[j] * coord_of(sv[k], j);
                } else {
                    const int64_t ii = (i < n) ? i : 0;
                    for (int j = 0; j < d; ++j) q += zt[offset_of(j) + ii * 128] * coord_of(sv[k], j);
                }
                buf[k * 64 + lane] = (k < K && i <= t + k) ? 0.5 * fabs(q - yr) : 0.0;
            }
            __builtin_amdgcn_wave_barrier();
            int u = 0;
            for (; u + 4 <= m; u += 4) {
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int k = 0; k < kSpec; ++k) out[k] += buf[k * 64 + u + v];
            }
            for (; u < m; ++u)
#pragma unroll
                for (int k = 0; k < kSpec; ++k) out[k] += buf[k * 64 + u];
            __builtin_amdgcn_wave_barrier();
        };
        if constexpr (DMAX > 0) {
            double zc[DMAX], yc = 0.0;
            auto load = [&](int64_t i0, double (&zb)[DMAX], double& yb) {
                const int64_t i = (i0 + lane < n) ? i0 + lane : 0;
#pragma unroll
                for (int j = 0; j < DMAX; ++j) zb[j] = (j < d) ? zt[offset_of(j) + i * 128] : 0.0;
                yb = yp[i * S];
            };
            load(0, zc, yc);
            for (int64_t i0 = 0; i0 < n; i0 += 64) {
                double zn[DMAX], yn = 0.0;
                if (i0 + 64 < n) load(i0 + 64, zn, yn);
                chunk(i0, zc, yc);
#pragma unroll
                for (int j = 0; j < DMAX; ++j) zc[j] = zn[j];
                yc = yn;
            }
        } else {
            for (int64_t i0 = 0; i0 < n; i0 += 64) {
                const int64_t i = (i0 + lane < n) ? i0 + lane : 0;
                chunk(i0, nullptr, yp[i * S]);
            }
        }
    };

    // shared by the columns
    double tf = 0.0;  // theta_ftl (coordinate `lane`)
    double ftl_loss = 0.0;
    unsigned long long tested = 0;
    // per column; spare columns (m >= nt) are never live
    double th[NT], tr[NT], total[NT];  // threshold, theta_ftrl (coordinate `lane`), own total
    bool switched[NT];
    int64_t sw[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        th[m] = (m < nt) ? a.thresh[b * a.M + a.m0 + m] : 0.0;
        tr[m] = total[m] = 0.0;
        switched[m] = false;
        sw[m] = -1;
    }
    // FTRL step tk (:148-154) of the NT columns side by side, on the row (z, yv) the FTL leg
    // of that step has loaded, committed where act[m]
    auto ftrl_steps = [&](int64_t tk, double z, double yv, const bool (&act)[NT]) {
        const double sc = -(eta0 / sqrt((double)(tk + 1)));
        double xr[NT], v[NT], n2[NT], pr[NT];
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            xr[m] = sc * tr[m];
            v[m] = own ? xr[m] * xr[m] : 0.0;
        }
        ordered_sum_grid_cols<NT>(v, d, buf, lane, n2);
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            if (n2[m] > 1.0) xr[m] *= 1.0 / sqrt(n2[m]);
            v[m] = own ? z * xr[m] : 0.0;
        }
        ordered_sum_grid_cols<NT>(v, d, buf, lane, pr);
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            if (act[m]) {
                const double dr = pr[m] - yv;
                total[m] += 0.5 * fabs(dr);
                tr[m] += grad(dr) * z;
            }
        }
    };
    // checkpoint k, wave-uniform, inside the batch (curve_next: [0, T + 1])
    auto checkpoint = [&](int64_t k) -> int64_t {
        const int64_t v = curve_next<int64_t>(a.ck, a.K, T, k);
        return v > T ? T : v;
    };

    double xf_next = 0.0;  // FTL(theta_ftl) as it stands: FTL(0) = 0
    int64_t kc = 0;        // the next checkpoint's index
    int64_t t = 0;
    int64_t hn = checkpoint(0);
    while (kc < a.K) {
        if (hn <= t) {
            // the emission at checkpoint hn (= t): comparator = FTL(theta_ftl) on rows
            // 0 … hn − 1 (:162-163), once for all columns
            const double comp = prefix_loss(action_ftl(tf, d, buf, lane), hn);
            if (lane == 0) {
#pragma unroll
                for (int m = 0; m < NT; ++m) {
                    if (m < nt) {
                        const int64_t o = (b * a.M + a.m0 + m) * a.K + kc;
                        // a column that has not switched: total_loss is ftl_loss (:156)
                        a.regret[o] = (switched[m] ? total[m] : ftl_loss) - comp;
                        if (a.switch_step) a.switch_step[o] = sw[m];
                    }
                }
            }
            ++kc;
            hn = checkpoint(kc);
            continue;
        }
        bool live[NT];
        bool anyun = false;
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            live[m] = m < nt;
            anyun = anyun || (live[m] && !switched[m]);
        }
        if (!anyun) {
            // every live column has switched: the single kernel's post-switch step (:140-154),
            // FTL still updated, FTRL played with each column's own theta
            const double z = own ? zt[zoff + t * 128] : 0.0;
            const double yv = yp[t * S];
            const double xf = action_ftl(tf, d, buf, lane);
            const double pf = ordered_sum(0.0, own ? z * xf : 0.0, d, buf, lane);
            const double dfl = pf - yv;
            tf += grad(dfl) * z;
            ftl_loss += 0.5 * fabs(dfl);
            ftrl_steps(t, z, yv, live);
            ++t;
            continue;
        }
        // Pre-switch steps go kSpec at a time: the FTL part of each step (which never depends
        // on the switch) runs ahead, the kSpec prefix re-scans run side by side, and the
        // switch test is then applied per column in step order.
        const int K = (hn - t) < kSpec ? (int)(hn - t) : kSpec;
        double sv[kSpec], fl[kSpec], zk[kSpec], yk[kSpec];
#pragma unroll
        for (int k = 0; k < kSpec; ++k) {
            sv[k] = 0.0;
            fl[k] = 0.0;
            zk[k] = yk[k] = 0.0;
            if (k < K) {
                const double z = zk[k] = own ? zt[zoff + (t + k) * 128] : 0.0;
                const double yv = yk[k] = yp[(t + k) * S];
                const double pf = ordered_sum(0.0, own ? z * xf_next : 0.0, d, buf, lane);
                const double dfl = pf - yv;
                tf += grad(dfl) * z;
                ftl_loss += 0.5 * fabs(dfl);
                fl[k] = ftl_loss;
                sv[k] = action_ftl(tf, d, buf, lane);  // s_{t+k} (:157), the next FTL action
                xf_next = sv[k];
            }
        }
        double sl[kSpec];
        prefix_loss_multi(sv, t, K, sl);
        bool before[NT];  // switched before this group
        int ks[NT];       // the group's step at which the column switches, or -1
        int steps = 0;    // steps of the group whose test some column needed
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            before[m] = live[m] && switched[m];
            ks[m] = -1;
            if (live[m] && !switched[m]) {
#pragma unroll
                for (int k = 0; k < kSpec; ++k) {
                    if (k < K && ks[m] < 0 && fl[k] - sl[k] >= th[m]) {
                        ks[m] = k;
                        total[m] = fl[k];  // the additions of `total_loss += lf` so far (:156)
                    }
                }
                if (ks[m] >= 0) {
                    switched[m] = true;
                    sw[m] = t + ks[m];
                }
                const int c = ks[m] >= 0 ? ks[m] + 1 : K;
                steps = c > steps ? c : steps;
            }
        }
        tested += (unsigned long long)steps;
        // FTRL on the group's steps: all of them for a column switched before the group, the
        // steps after its switch for one that switched inside it
#pragma unroll 1
        for (int k = 0; k < K; ++k) {  // one copy of the step: the row is picked by selects
            bool act[NT];
            bool any = false;
#pragma unroll
            for (int m = 0; m < NT; ++m) {
                act[m] = before[m] || (ks[m] >= 0 && k > ks[m]);
                any = any || act[m];
            }
            double z = zk[0], yv = yk[0];
#pragma unroll
            for (int u = 1; u < kSpec; ++u) {
                z = (k == u) ? zk[u] : z;
                yv = (k == u) ? yk[u] : yv;
            }
            if (any) ftrl_steps(t + k, z, yv, act);
        }
        t += K;
    }
    if (lane == 0 && a.stats && tested) atomicAdd(&a.stats[0], tested);
}

namespace {

template <int NT>
hipError_t launch_wave_grid(const WaveGridArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.B + (kGridBlock / 64) - 1) / (kGridBlock / 64));
    if (a.d <= 8) {
        hipLaunchKernelGGL((ocx_smart_wave_grid_kernel<8, NT>), dim3(grid), dim3(kGridBlock), 0,
                           st, a);
    } else if constexpr (NT > 1) {
        hipLaunchKernelGGL((ocx_smart_wave_grid_kernel<0, NT>), dim3(grid), dim3(kGridBlock), 0,
                           st, a);
    } else {
        return hipErrorInvalidValue;  // not compiled: the caller takes the two-column instance
    }
    return hipGetLastError();
}

}  // namespace

bool ocx_smart_wave_grid_instance(int group) {
    return group == 1 || group == 2 || group == 4 || group == 8;
}

hipError_t ocx_launch_smart_wave_grid(const ocx_layout* L, const double* zt, const double* yt,
                                      const double* th, int64_t M, const int64_t* ck, int64_t K,
                                      double eta0, double* reg, int64_t* sw,
                                      unsigned long long* stats, int group, hipStream_t st) {
    if (L->B == 0 || M <= 0 || K <= 0) return hipSuccess;
    if (L->d > 64) return hipErrorNotSupported;
    if (!ocx_smart_wave_grid_instance(group)) return hipErrorInvalidValue;
    WaveGridArgs a{zt, yt, L->B, L->T, (int)L->d, L->P, L->C, L->G, th, M, /*m0*/ 0, /*nt*/ 0,
                   ck, K, eta0, reg, sw, stats};  // m0, nt: per launch
    for (int64_t m0 = 0; m0 < M; m0 += group) {
        const int nt = (int)(M - m0 < group ? M - m0 : group);
        a.m0 = m0;
        a.nt = nt;
        // the smallest instance that holds them; above d = 8 a single column runs on the
        // two-column instance with a spare column (the one-column instance of the DMAX = 0 row
        // path needs 132 VGPRs, three waves per SIMD where the column kernel's runs four on
        // 128, and is not compiled: profiles/smart_grid_resource_usage.txt)
        const hipError_t e = (nt <= 1 && a.d <= 8) ? launch_wave_grid<1>(a, st)
                             : nt <= 2 ? launch_wave_grid<2>(a, st)
                             : nt <= 4 ? launch_wave_grid<4>(a, st)
                                       : launch_wave_grid<8>(a, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
