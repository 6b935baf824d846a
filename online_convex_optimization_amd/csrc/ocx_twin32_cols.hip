// ocx_twin32_cols.hip — the float32 twin (algorithms.py) for up to NT columns (horizon t_k,
// algorithm, threshold) per staging of a sequence's rows and per prefix re-scan: the NT-column
// form of ocx_twin32_smart_wave_kernel (ocx_twin32.hip).  Column k carries the bits of
// ocx_dev_twin32(algo_k, eta0, thresh[:, k]) on a batch of the first t_k rows.
//
// Why one re-scan serves every column.  SMART's pre-switch test at step t (algorithms.py:
// 109-111) computes sl = np.sum(0.5 * np.abs(z[:t+1] @ FTL(theta_{t+1}) - y[:t+1])): the
// comparator loss (:51-53, :116-118) of a run truncated at horizon t + 1 — the same function
// of the same arguments, the row count n = t + 1 that picks sgemv's row rule included.  The
// FTL trajectory depends on neither the threshold nor the horizon, and simulate_alg's FTL
// (algo 1) is the SMART column that never switches: the same adds into the loss from 0.0, the
// same comparator.  So per wave there is ONE FTL theta and loss, ONE FTRL-from-step-0 theta and
// loss (all algo-0 columns; advanced to their last horizon only), and at most ONE
// t32_wave_loss_sum per step for sl, made iff some live SMART column is unswitched or a column
// of algorithm 1 / 2 freezes at t + 1.  A column owns its FTRL-after-switch theta, its loss
// since the switch, its switch step and two flags.
//
// A column freezes when t reaches t_k: its loss as it stands; comparator = the sl of step
// t_k - 1 for FTL and SMART columns; for an FTRL column one extra re-scan with FTL(theta of the
// FTRL run) at n = t_k — simulate_alg's comparator comes from that run's own theta
// (ocx_twin32_kernel's last lines), once for all FTRL columns at that horizon.  The horizons
// are non-decreasing; the loop ends at the launch's last one, and only rows [0, t_last) are
// staged.  Horizon 0 gives 0.0f, 0.0, 0.0f and -1.
//
// One wavefront per sequence, every lane holding the same scalars, as in the single kernel:
// horizons, algorithms and flags come by value in the kernel arguments and the thresholds are
// read at a wave-uniform address, so every branch around t32_wave_loss_sum (which contains
// __syncthreads()) is wave-uniform.  The arithmetic is ocx_twin32.h's, one copy for both files.
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"
#include "ocx_twin32.h"

namespace {

constexpr int kT32MaxCols = 8;  // the widest instance

struct T32ColsArgs {
    const double* zt;
    const double* yt;
    int64_t T, G;      // of the batch's layout (strides)
    int64_t K, k0;     // row stride of thresh and the outputs, first column of this launch
    int nt;            // columns of this launch (<= the instance's NT)
    int t_last;        // h[nt - 1]: rows staged, steps run
    int t_ftrl;        // the last horizon of an algo-0 column (0: none)
    int h[kT32MaxCols];     // horizons, non-decreasing in [0, T]
    int algo[kT32MaxCols];  // 0 FTRL, 1 FTL, 2 SMART
    double eta0;
    const double* thresh;  // [B][K], read for SMART columns only
    float* result;         // [B][K]
    double* cum;           // [B][K], nullable
    float* comp;           // [B][K], nullable
    int64_t* sw;           // [B][K], nullable
};

// columns per launch that keep NT * C <= 64 floats of per-column theta
constexpr int t32_cols_max(int C) { return C <= 8 ? 8 : (C <= 16 ? 4 : 2); }

}  // namespace

template <int C, int NT>
__global__ __launch_bounds__(64) void ocx_twin32_cols_kernel(T32ColsArgs a) {
    extern __shared__ float t32c_lds[];
    __shared__ float red[64];
    __shared__ int lstart[kWaveLeaves], llen[kWaveLeaves];
    __shared__ float lsum[kWaveLeaves];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int n = a.t_last, nt = a.nt;
    float* zs = t32c_lds;
    float* ys = t32c_lds + (int64_t)n * C;
    {
        // stage rows [0, t_last) of the sequence (lane sl of wave-group g in the P = 1 layout)
        const int64_t g = b / 64;
        const int sl = (int)(b % 64);
        const ocx_d2* zp = reinterpret_cast<const ocx_d2*>(a.zt) + g * a.T * 64 + sl;
        const int64_t kst = a.G * a.T * 64;
        for (int t = lane; t < n; t += 64) {
#pragma unroll
            for (int k = 0; k < C / 2; ++k) {
                const ocx_d2 v = zp[(int64_t)t * 64 + k * kst];
                zs[t * C + 2 * k] = (float)v.x;
                zs[t * C + 2 * k + 1] = (float)v.y;
            }
            ys[t] = (float)a.yt[(g * a.T + t) * 64 + sl];
        }
    }
    __syncthreads();
    T32Wave w{zs, ys, red, lstart, llen, lsum};
    const double eta0 = a.eta0;
    // shared by the columns
    float th[C], tf[C], x[C], sx[C];  // theta of FTL and of FTRL from step 0
    double ftl_loss = 0.0, ftrl_loss = 0.0;
    // per column; the spare columns of a tail launch (m >= nt) start frozen
    float thr[NT][C], th32[NT];
    double cum[NT];
    unsigned swm = 0, frm = 0;  // bit m: column m has switched / is frozen
    int sw[NT];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = tf[j] = 0.0f;
#pragma unroll
    for (int m = 0; m < NT; ++m) {
#pragma unroll
        for (int j = 0; j < C; ++j) thr[m][j] = 0.0f;
        th32[m] = (m < nt && a.algo[m] == 2) ? (float)a.thresh[b * a.K + a.k0 + m] : 0.0f;
        cum[m] = 0.0;
        if (m >= nt) frm |= 1u << m;
        sw[m] = -1;
    }
    auto emit = [&](int m, double c, float comp, int64_t s) {
        if (lane == 0) {
            const int64_t o = b * a.K + a.k0 + m;
            a.result[o] = (float)c - comp;
            if (a.cum) a.cum[o] = c;
            if (a.comp) a.comp[o] = comp;
            if (a.sw) a.sw[o] = s;
        }
    };
#pragma unroll
    for (int m = 0; m < NT; ++m)
        if (!(frm >> m & 1u) && a.h[m] == 0) {
            emit(m, 0.0, 0.0f, -1);
            frm |= 1u << m;
        }
    for (int t = 0; t < n; ++t) {
        float zr[C];
#pragma unroll
        for (int j = 0; j < C; ++j) zr[j] = zs[t * C + j];
        const double yv = (double)ys[t];
        // the FTL leg (simulate_alg's FTL step; simulate_SMART_like :84-93)
        t32_ftl<C>(th, x);
        const double pf = (double)t32_sdot<C>(zr, x);
        const float gf = (float)t32_grad(pf - yv);
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = th[j] + gf * zr[j];
        ftl_loss += 0.5 * fabs(pf - yv);
        // FTRL from step 0 (simulate_alg, algo 0)
        if (t < a.t_ftrl) {
            t32_ftrl<C>(tf, t + 1, eta0, x);
            const double pr = (double)t32_sdot<C>(zr, x);
            ftrl_loss += 0.5 * fabs(pr - yv);
            const float gr = (float)t32_grad(pr - yv);
#pragma unroll
            for (int j = 0; j < C; ++j) tf[j] = tf[j] + gr * zr[j];
        }
        // FTRL after the switch, per column; does anything need this step's prefix loss?
        bool need = false, ftrl_freezes = false;
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            if (frm >> m & 1u) continue;
            if (a.algo[m] == 2) {
                if (swm >> m & 1u) {
                    t32_ftrl<C>(thr[m], t + 1, eta0, x);
                    const double pr = (double)t32_sdot<C>(zr, x);
                    cum[m] += 0.5 * fabs(pr - yv);
                    const float gr = (float)t32_grad(pr - yv);
#pragma unroll
                    for (int j = 0; j < C; ++j) thr[m][j] = thr[m][j] + gr * zr[j];
                } else {
                    need = true;
                }
            }
            if (a.h[m] == t + 1) {
                if (a.algo[m] == 0)
                    ftrl_freezes = true;
                else
                    need = true;
            }
        }
        // pass 0: sl, the prefix loss of FTL(theta_ftl); pass 1: the comparator of the FTRL run,
        // FTL of its own theta (one copy of the wave sum in the code)
        float sl = 0.0f, fcomp = 0.0f;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            if (!(pass == 0 ? need : ftrl_freezes)) continue;
            if (pass == 0)
                t32_ftl<C>(th, sx);
            else
                t32_ftl<C>(tf, sx);
            const float v = t32_wave_loss_sum<C>(w, sx, t + 1, lane);
            if (pass == 0)
                sl = v;
            else
                fcomp = v;
        }
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            if (frm >> m & 1u) continue;
            if (a.algo[m] == 2 && !(swm >> m & 1u) && (float)ftl_loss - sl >= th32[m]) {
                swm |= 1u << m;
                sw[m] = t;
                cum[m] = ftl_loss;  // total_loss += lf so far: the same adds from 0.0
            }
            if (a.h[m] == t + 1) {
                if (a.algo[m] == 0)
                    emit(m, ftrl_loss, fcomp, -1);
                else
                    emit(m, (swm >> m & 1u) ? cum[m] : ftl_loss, sl, sw[m]);
                frm |= 1u << m;
            }
        }
    }
}

namespace {

template <int C, int NT>
hipError_t launch_t32_cols_nt(const T32ColsArgs& a, int64_t B, hipStream_t st) {
    if constexpr (NT > t32_cols_max(C)) {
        return hipErrorInvalidValue;
    } else {
        const size_t lds = (size_t)a.t_last * (C + 1) * 4;
        hipLaunchKernelGGL((ocx_twin32_cols_kernel<C, NT>), dim3((unsigned)B), dim3(64), lds, st, a);
        return hipGetLastError();
    }
}

template <int C>
hipError_t launch_t32_cols(const ocx_layout* L, const double* zt, const double* yt, int64_t K,
                           const int64_t* hz, const int32_t* algos, double eta0,
                           const double* thresh, float* result, double* cum, float* comp,
                           int64_t* sw, int group, hipStream_t st) {
    if (group > t32_cols_max(C)) return hipErrorInvalidValue;
    T32ColsArgs a{zt, yt, L->T, L->G, K, 0, 0, 0, 0, {}, {}, eta0, thresh, result, cum, comp, sw};
    for (int64_t k0 = 0; k0 < K; k0 += group) {
        const int nt = (int)(K - k0 < group ? K - k0 : group);
        a.k0 = k0;
        a.nt = nt;
        a.t_ftrl = 0;
        for (int m = 0; m < kT32MaxCols; ++m) {
            const int64_t k = k0 + (m < nt ? m : nt - 1);
            a.h[m] = (int)hz[k];
            a.algo[m] = algos[k];
            if (m < nt && algos[k] == 0) a.t_ftrl = (int)hz[k];
        }
        a.t_last = a.h[nt - 1];
        // the smallest instance that holds them
        const hipError_t e = nt <= 1   ? launch_t32_cols_nt<C, 1>(a, L->B, st)
                             : nt <= 2 ? launch_t32_cols_nt<C, 2>(a, L->B, st)
                             : nt <= 4 ? launch_t32_cols_nt<C, 4>(a, L->B, st)
                                       : launch_t32_cols_nt<C, 8>(a, L->B, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

// the widest group of the layout's instance: NT * C <= 64 floats of per-column theta
int ocx_twin32_cols_max_group(const ocx_layout* L) { return t32_cols_max(L->C); }

// the longest horizon whose rows fit the LDS: t * (C + 1) * 4 <= kWaveLdsBytes
int64_t ocx_twin32_cols_max_horizon(const ocx_layout* L) {
    return kWaveLdsBytes / ((int64_t)(L->C + 1) * 4);
}

hipError_t ocx_launch_twin32_cols(const ocx_layout* L, const double* zt, const double* yt,
                                  int64_t K, const int64_t* hz, const int32_t* algos, double eta0,
                                  const double* thresh, float* result, double* cum, float* comp,
                                  int64_t* sw, int group, hipStream_t st) {
    if (L->B == 0 || K <= 0) return hipSuccess;
    if (L->P != 1 || L->S != 64) return hipErrorInvalidValue;
    if (group != 1 && group != 2 && group != 4 && group != 8) return hipErrorInvalidValue;
    if (hz[K - 1] > ocx_twin32_cols_max_horizon(L)) return hipErrorNotSupported;
    switch (L->C) {
#define OCX_T32_COLS_CASE(CC)                                                                     \
    case CC:                                                                                      \
        return launch_t32_cols<CC>(L, zt, yt, K, hz, algos, eta0, thresh, result, cum, comp, sw,  \
                                   group, st);
        OCX_T32_COLS_CASE(2)
        OCX_T32_COLS_CASE(4)
        OCX_T32_COLS_CASE(6)
        OCX_T32_COLS_CASE(8)
        OCX_T32_COLS_CASE(12)
        OCX_T32_COLS_CASE(16)
        OCX_T32_COLS_CASE(24)
        OCX_T32_COLS_CASE(32)
#undef OCX_T32_COLS_CASE
        default: return hipErrorInvalidValue;
    }
}
