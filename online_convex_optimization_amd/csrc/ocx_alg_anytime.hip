// ocx_alg_anytime.hip — anytime regret: the running max of FTRL/FTL's regret over EVERY prefix
// t = 1 … T of a sequence (fast_algorithms.py:88-115 applied to each prefix), in one pass.
//
// The curve kernels (ocx_alg_curve.hip) stop at K checkpoints and leave a workspace slot per
// (wave-group, checkpoint) for the streamed comparator; a dense curve (K = T) fits neither in
// time nor in memory.  Where the closed-form comparator is certified, the regret of the prefix
// of t rows is R_t = cum_t − (t/2 − ||θ_t||), and θ_t and cum_t are in registers at the top of
// every step of both loops — exactly the state CurveObserver receives.  AnytimeObserver is an
// observer of the same interface that evaluates the closed form at every step instead of at K of
// them: one fresh norm per step (C products, one ocx_total, one sqrt), no workspace, no second
// kernel.  Its loops are the curve's: alg_pipe_body (ocx_alg_pipe.h) where the pipelined form
// runs, and a plain kernel over ocx_plain_step (ocx_alg_step.h) for every other layout, the
// chained exact ones included.  The helper (ocx_closed_comp) and the arithmetic are
// curve_emit's, so R_t carries the bits of column t of a dense curve.
//
// Per step t = 1 … T (t < T at the top of loop step t, t = T after the loop), with th = θ_t,
// cum and clean covering steps 0 … t-1:
//   closed = onepass && (clean || !live)              curve_emit's rule; monotone in t
//   r      = cum − (t/2 − ||θ_t||)                    where closed
//   closed:  if (r > best) { best = r; arg = t; }     strict: the smallest t wins a tie
//   !closed: the first such t is open_from; nothing after it enters best, arg or the trace
// and at each checkpoint t_k (device int64 [K], strictly increasing in [1, T], walked through
// curve_next on the scalar unit as the curve does) lane c == 0 of a live sequence stores
// (best, arg) at [b][k].  With TRACE, r (NaN where not closed) goes to
// trace[(g·T + (t-1))·S + s], y_tiled's layout.
//
// Whatever the checkpoint array holds, every access stays inside the batch and the outputs:
// the emission index runs over [0, K) once, and rows and trace slots are addressed by the step
// counter.  Padding sequences (b >= B) write nothing.
#include <limits>

#include "ocx_alg_pipe.h"
#include "ocx_alg_step.h"
#include "ocx_curve_ck.h"
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

struct AnytimeArgs {
    PipeArgs p;  // the batch; a whole run of every group (its own outputs stay null)
    int ftl;
    const int64_t* ck;  // device [K]
    int64_t K;
    double* sup;         // [B][K], nullable
    int64_t* argsup;     // [B][K], nullable
    int64_t* open_from;  // [B], nullable
    double* trace;       // y_tiled's layout, read by the TRACE instances only
};

// The per-step observer of both loops (CurveObserver's interface).  IT: the loop's step type —
// the checkpoint comparison stays on the scalar unit, and arg / open take one register each
// where the loop counts in int.  TRACE: a template flag, so the address arithmetic and the
// store of the trace cost the hot instance nothing.
template <int C, int P, bool CHAIN, class IT, bool TRACE>
struct AnytimeObserver {
    static constexpr int S = 64 / P;
    const AnytimeArgs& a;
    int64_t k;
    IT nxt;
    double best;  // max of R_t over the certified steps so far
    IT arg;       // the smallest t attaining it; 0: none yet
    IT open;      // the first t whose prefix was not certified; 0: none yet
    __device__ __forceinline__ explicit AnytimeObserver(const AnytimeArgs& a_)
        : a(a_), k(0), nxt(curve_next<IT>(a_.ck, a_.K, a_.p.T, 0)),
          best(-std::numeric_limits<double>::infinity()), arg(0), open(0) {}

    // horizon t >= 1, th = θ_t.  Whole wave active (lane exchanges).
    __device__ __forceinline__ void observe(int64_t t, int64_t g, int64_t b, int c, int lane,
                                            bool live, const double (&th)[C], double cum,
                                            bool clean) {
        const bool closed = a.p.onepass && (clean || !live);
        double comp = 0.0;
        ocx_closed_comp<C, P, CHAIN>(th, closed, t, comp, lane);
        const double r = cum - comp;
        if (closed) {
            if (r > best) {
                best = r;
                arg = (IT)t;
            }
        } else if (open == 0) {
            open = (IT)t;
        }
        if constexpr (TRACE) {
            if (c == 0 && live)
                a.trace[(g * a.p.T + (t - 1)) * S + lane / P] = closed ? r : __builtin_nan("");
        }
    }
    __device__ __forceinline__ void emit(int64_t b, int c, bool live) {
        if (c == 0 && live) {
            const int64_t o = b * a.K + k;
            if (a.sup) a.sup[o] = best;
            if (a.argsup) a.argsup[o] = (int64_t)arg;
        }
    }
    __device__ __forceinline__ void step(int64_t t, int64_t g, int64_t b, int c, int lane, bool live,
                                         const double (&th)[C], double cum, bool clean) {
        if ((IT)t == 0) return;  // wave-uniform: θ_0 belongs to no prefix
        observe(t, g, b, c, lane, live, th, cum, clean);
        while ((IT)t >= nxt) {  // wave-uniform
            emit(b, c, live);
            ++k;
            nxt = curve_next<IT>(a.ck, a.K, a.p.T, k);
        }
    }
    __device__ __forceinline__ void finish(int64_t g, int64_t b, int c, int lane, bool live,
                                           const double (&th)[C], double cum, bool clean) {
        const int64_t T = a.p.T;
        if (T > 0) observe(T, g, b, c, lane, live, th, cum, clean);
        while (k < a.K) {
            emit(b, c, live);
            ++k;
        }
        if (c == 0 && live && a.open_from) a.open_from[b] = open != 0 ? (int64_t)open : T + 1;
    }
};

}  // namespace

// ---------------------------------------------------------------------------
// The plain form (the shape of ocx_alg_curve_kernel): every layout the pipelined form does not
// take, the chained exact layouts included.
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB, bool TRACE>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_alg_anytime_kernel(AnytimeArgs a) {
    const int64_t g = ocx_wave_id();
    if (g >= a.p.G) return;
    const int64_t T = a.p.T;
    const OcxSeq<P> q(a.p.zt, a.p.yt, g, a.p.B, T, a.p.G);
    const int lane = q.lane;
    const bool check = ocx_check_rows(a.p.onepass);
    const double eta0 = a.p.eta0;
    const bool ftl = a.ftl != 0;
    bool clean = true;  // every row in the ball, every sub-gradient −y_t/2 so far

    double th[C];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = 0.0;

    ocx_d2 zb[NB][C / 2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], q.zp + tl * 64, q.kst);
        yb[slot] = q.yp[tl * q.S];
    };

    double cum = 0.0;
    AnytimeObserver<C, P, CHAIN, int64_t, TRACE> obs(a);
    OcxScaleTable sct;  // FTRL scales, 64 steps at a time
    ocx_ring_loop<NB>(T, load, [&](int u, int64_t t) {
        obs.step(t, g, q.b, q.c, lane, q.live, th, cum, clean);
        ocx_plain_step<C, P, CHAIN>(ftl, th, zb[u], yb[u], check, cum, clean, lane,
                                    [&] { return ocx_ftrl_scale(sct, t + 1, eta0, lane); });
    });
    obs.finish(g, q.b, q.c, lane, q.live, th, cum, clean);
}

// ---------------------------------------------------------------------------
// The pipelined form (whole runs): ocx_alg_pipe_kernel's loop (alg_pipe_body) with the observer,
// which also replaces its epilogue.
// ---------------------------------------------------------------------------
template <int C, int P, int NB, bool FTL, bool RT, bool TRACE>
__global__ __launch_bounds__(OCX_BLOCK, 1) void ocx_alg_pipe_anytime_kernel(AnytimeArgs a) {
    alg_pipe_body<C, P, NB, FTL, RT, false>(
        a.p, AnytimeObserver<C, P, false, pipe_step_t<C>, TRACE>(a));
}

// ---------------------------------------------------------------------------
// Launchers: ocx_launch_alg_curve's dispatch, launch policy and block shapes
// ---------------------------------------------------------------------------
namespace {

template <int C, int P, bool CH>
hipError_t launch_anytime_cp(const ocx_layout* L, const AnytimeArgs& a, hipStream_t st) {
    const int bw = ocx_block_waves(L->G);
    const dim3 grid = ocx_grid(L->G, bw), block(64 * bw);
    if (a.trace)
        hipLaunchKernelGGL((ocx_alg_anytime_kernel<C, P, CH, nb_for(C, P), true>), grid, block, 0,
                           st, a);
    else
        hipLaunchKernelGGL((ocx_alg_anytime_kernel<C, P, CH, nb_for(C, P), false>), grid, block, 0,
                           st, a);
    return hipGetLastError();
}

template <int C, int P, bool FTL>
void launch_pipe_anytime_f(const AnytimeArgs& a, dim3 grid, dim3 block, hipStream_t st) {
    constexpr int NB = pipe_nb<C>(P);
    constexpr bool RT = pipe_rt<C, P, 1>();
    if (a.trace)
        hipLaunchKernelGGL((ocx_alg_pipe_anytime_kernel<C, P, NB, FTL, RT, true>), grid, block, 0,
                           st, a);
    else
        hipLaunchKernelGGL((ocx_alg_pipe_anytime_kernel<C, P, NB, FTL, RT, false>), grid, block, 0,
                           st, a);
}

template <int C, int P>
hipError_t launch_pipe_anytime_cp(const ocx_layout* L, const AnytimeArgs& a, hipStream_t st) {
    const int bw = pipe_block_waves(L->G);
    const dim3 grid = ocx_grid(L->G, bw), block(64 * bw);
    if (a.ftl) launch_pipe_anytime_f<C, P, true>(a, grid, block, st);
    else launch_pipe_anytime_f<C, P, false>(a, grid, block, st);
    return hipGetLastError();
}

hipError_t launch_pipe_anytime(const ocx_layout* L, const AnytimeArgs& a, hipStream_t st) {
    return ocx_pipe_dispatch(L, [&](auto c, auto p) {
        return launch_pipe_anytime_cp<decltype(c)::value, decltype(p)::value>(L, a, st);
    });
}

hipError_t launch_plain_anytime(const ocx_layout* L, const AnytimeArgs& a, hipStream_t st) {
    OCX_DISPATCH(launch_anytime_cp, L, a, st)
}

}  // namespace

hipError_t ocx_launch_alg_anytime(const ocx_layout* L, const double* zt, const double* yt, int ftl,
                                  double eta0, const int64_t* ck, int64_t K, double* sup,
                                  int64_t* argsup, int64_t* open_from, double* trace, int onepass,
                                  hipStream_t st) {
    if (L->G == 0 || L->T <= 0) return hipSuccess;
    AnytimeArgs a{};
    a.p.zt = zt;
    a.p.yt = yt;
    a.p.B = L->B;
    a.p.T = L->T;
    a.p.G = L->G;
    a.p.eta0 = eta0;
    a.p.onepass = onepass;
    a.p.gn = L->G;  // every group, the whole horizon
    a.p.tn = L->T;
    a.ftl = ftl;
    a.ck = ck;
    a.K = K;
    a.sup = sup;
    a.argsup = argsup;
    a.open_from = open_from;
    a.trace = trace;
    return ocx_alg_use_pipe(L) ? launch_pipe_anytime(L, a, st) : launch_plain_anytime(L, a, st);
}
