// ocx_alg_curve.hip — regret curves: FTRL/FTL (fast_algorithms.py:88-115) observed at K
// checkpoint horizons t_1 < … < t_K <= T in one pass over a sequence of T steps.
//
// FTRL and FTL are online: the first t steps of a run on (z, y) are the run on
// (z[:t], y[:t]).  So the loop of a whole-horizon run passes through the state every
// truncated run would end in, and a curve needs only that the loop stops there and
// evaluates the comparator of the prefix: the loss of FTL(θ_t) over rows 0 … t-1
// (fast_algorithms.py:113-115 applied to the prefix).
//
// Two loop kernels, the curve forms of ocx_alg_kernel (ocx_sim.hip) and of the pipelined
// butterfly kernel (ocx_alg_pipe.hip), dispatched by ocx_launch_alg's rule.  The pipelined
// form is the parent's own loop (alg_pipe_body, ocx_alg_pipe.h) with an observer; the plain
// form's loop body is the shared plain step (ocx_plain_step, ocx_alg_step.h).  So column k of
// a curve carries the bits of a run of those kernels on the input truncated at t_k.
// The checkpoint list is wave-uniform: the kernels hold the next checkpoint in a scalar and
// compare it with the step counter once per step.  At the top of step t == t_k, once `th`
// holds θ_{t_k} (the plain kernel: as the step begins; the pipelined kernel: right after its
// lagging θ is brought up to date), they emit
//   - cum, the loss paid in steps 0 … t_k - 1;
//   - the certificate so far (`clean`: rows in the ball, labels ±1, sub-gradients −y/2);
//   - where the closed form is requested and certified, t_k/2 − ||θ_{t_k}||, the norm summed
//     afresh from θ as the parents' epilogues do.
// t_k = T is emitted after the loop.
//
// A pair (sequence, checkpoint) that does not take the closed form still owes the reference's
// streamed comparator pass over its prefix.  The loop does not re-scan (its register ring
// holds the look-ahead rows): it leaves θ_{t_k}, each lane its own C coordinates, and cum in
// the caller's workspace, and ocx_curve_comp_kernel — one wave per (wave-group, checkpoint) —
// streams rows 0 … t_k - 1 with x* = FTL(θ_{t_k}) in the summation order of the parents'
// second passes.  A wave none of whose sequences needs it exits after one 256-byte read, so a
// certified batch reads z once; otherwise the extra reads are the prefixes of the uncertified
// pairs only.  A certified sequence keeps the closed form whatever its wave neighbours do.
//
// Workspace for K checkpoints (ocx_curve_ws_bytes), slot = g·K + k:
//   θ     [G·K][C][64] doubles   word j of lane l at ((slot·C + j)·64 + l): coalesced
//   cum   [G·K][64]    doubles
//   need  [G·K][64]    int32     1: the lane's sequence takes the streamed pass
//
// The checkpoint array lives in device memory and its order is the caller's precondition.
// Whatever it holds, every access stays inside the batch, the outputs and the workspace: the
// emission index k runs over [0, K) exactly once, rows are addressed by the step counter, and
// the comparator pass clamps its horizon to [0, T].
#include "ocx_alg_pipe.h"
#include "ocx_alg_step.h"
#include "ocx_curve_ck.h"
#include "ocx_device_math.h"
#include "ocx_dispatch.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

namespace {

struct CurveArgs {
    PipeArgs p;  // the batch and the outputs ([B][K], each nullable); a whole run of every group
    int ftl;
    const int64_t* ck;  // device [K]
    int64_t K;
    double* ws_theta;
    double* ws_cum;
    int* ws_need;
};

// checkpoint k as the loop's step type (curve_ck / curve_next: ocx_curve_ck.h)
template <class IT>
__device__ __forceinline__ IT curve_next(const CurveArgs& a, int64_t k) {
    return ::curve_next<IT>(a.ck, a.K, a.p.T, k);
}

// Emission of checkpoint k at horizon tk, th = θ_{tk}.  Whole wave active (lane exchanges).
template <int C, int P, bool CHAIN>
__device__ __forceinline__ void curve_emit(const CurveArgs& a, int64_t g, int64_t k, int64_t tk,
                                           const double (&th)[C], double cum, bool clean,
                                           bool live, int64_t b, int c, int lane) {
    const bool closed = a.p.onepass && (clean || !live);
    double comp = 0.0;
    ocx_closed_comp<C, P, CHAIN>(th, closed, tk, comp, lane);
    const int64_t slot = g * a.K + k;
    a.ws_need[slot * 64 + lane] = closed ? 0 : 1;
    a.ws_cum[slot * 64 + lane] = cum;
    if (__ballot(!closed) != 0) {  // θ for the streamed pass of this wave's uncertified pairs
#pragma unroll
        for (int j = 0; j < C; ++j) a.ws_theta[(slot * C + j) * 64 + lane] = th[j];
    }
    if (c == 0 && live) {
        const int64_t o = b * a.K + k;
        if (a.p.cum_out) a.p.cum_out[o] = cum;
        if (a.p.closed_out) a.p.closed_out[o] = closed ? 1 : 0;
        if (closed) {  // the others: ocx_curve_comp_kernel
            if (a.p.comp_out) a.p.comp_out[o] = comp;
            if (a.p.regret) a.p.regret[o] = cum - comp;
        }
    }
}

// The per-step observer of both loops: emits the checkpoints met at step t (th = θ_t, cum and
// clean cover the steps before t), and after the loop t_k = T and whatever an unordered list
// left over.  IT: the loop's step type (the comparison stays on the scalar unit).
template <int C, int P, bool CHAIN, class IT>
struct CurveObserver {
    const CurveArgs& a;
    int64_t k;
    IT nxt;
    __device__ __forceinline__ explicit CurveObserver(const CurveArgs& a_)
        : a(a_), k(0), nxt(curve_next<IT>(a_, 0)) {}
    __device__ __forceinline__ void step(int64_t t, int64_t g, int64_t b, int c, int lane, bool live,
                                         const double (&th)[C], double cum, bool clean) {
        while ((IT)t >= nxt) {  // wave-uniform
            curve_emit<C, P, CHAIN>(a, g, k, t, th, cum, clean, live, b, c, lane);
            ++k;
            nxt = curve_next<IT>(a, k);
        }
    }
    __device__ __forceinline__ void finish(int64_t g, int64_t b, int c, int lane, bool live,
                                           const double (&th)[C], double cum, bool clean) {
        while (k < a.K) {
            curve_emit<C, P, CHAIN>(a, g, k, a.p.T, th, cum, clean, live, b, c, lane);
            ++k;
        }
    }
};

}  // namespace

// ---------------------------------------------------------------------------
// Curve form of ocx_alg_kernel (algo 0 / 1, no caller comparator): every layout the
// pipelined form does not take, the chained exact layouts included.  Its own loop — without
// x_last, the caller's comparator and the exact-FTL state its instances are smaller than the
// parent's — over the parent's step (ocx_plain_step).
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_alg_curve_kernel(CurveArgs a) {
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
    CurveObserver<C, P, CHAIN, int64_t> obs(a);
    OcxScaleTable sct;  // FTRL scales, 64 steps at a time
    ocx_ring_loop<NB>(T, load, [&](int u, int64_t t) {
        obs.step(t, g, q.b, q.c, lane, q.live, th, cum, clean);
        ocx_plain_step<C, P, CHAIN>(ftl, th, zb[u], yb[u], check, cum, clean, lane,
                                    [&] { return ocx_ftrl_scale(sct, t + 1, eta0, lane); });
    });
    obs.finish(g, q.b, q.c, lane, q.live, th, cum, clean);
}

// ---------------------------------------------------------------------------
// Curve form of the pipelined butterfly kernel (whole runs): ocx_alg_pipe_kernel's loop
// (alg_pipe_body, ocx_alg_pipe.h) with the observer, which also replaces its epilogue.
// ---------------------------------------------------------------------------
template <int C, int P, int NB, bool FTL, bool RT>
__global__ __launch_bounds__(OCX_BLOCK, 1) void ocx_alg_pipe_curve_kernel(CurveArgs a) {
    alg_pipe_body<C, P, NB, FTL, RT, false>(a.p, CurveObserver<C, P, false, pipe_step_t<C>>(a));
}

// ---------------------------------------------------------------------------
// The streamed comparator of the uncertified (sequence, checkpoint) pairs: wave w = g·K + k
// sums ½|z_t·x* − y_t| over rows 0 … t_k - 1 of wave-group g, x* = FTL(θ_{t_k}) from the
// workspace, in the order of the parents' second passes (ocx_comp_stream; ocx_comp_pass2 pairs
// the same additions).
// ---------------------------------------------------------------------------
template <int C, int P, bool CHAIN, int NB>
__global__ __launch_bounds__(OCX_BLOCK) void ocx_curve_comp_kernel(CurveArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = ocx_wave_id();
    if (w >= a.p.G * a.K) return;
    const int64_t g = w / a.K, k = w - g * a.K;
    const bool need = a.ws_need[w * 64 + lane] != 0;
    if (__ballot(need) == 0) return;  // wave-uniform: every pair of this wave is certified
    const int64_t T = a.p.T;
    int64_t tk = curve_ck(a.ck, k);
    tk = tk < 0 ? 0 : (tk > T ? T : tk);
    const OcxSeq<P> q(a.p.zt, a.p.yt, g, a.p.B, T, a.p.G);
    double th[C], xs[C];
#pragma unroll
    for (int j = 0; j < C; ++j) th[j] = a.ws_theta[(w * C + j) * 64 + lane];
    ocx_action_ftl<C, P, CHAIN>(th, xs, lane);
    ocx_d2 zb[NB][C / 2];
    double yb[NB];
    auto load = [&](int slot, int64_t tl) {
        ocx_load_tile<C>(zb[slot], q.zp + tl * 64, q.kst);
        yb[slot] = q.yp[tl * q.S];
    };
    const double comp = ocx_comp_stream<C, P, CHAIN, NB>(tk, load, zb, yb, xs, lane);
    if (need && q.c == 0 && q.live) {
        const int64_t o = q.b * a.K + k;
        if (a.p.comp_out) a.p.comp_out[o] = comp;
        if (a.p.regret) a.p.regret[o] = a.ws_cum[w * 64 + lane] - comp;
    }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
namespace {

template <int C, int P, bool CH>
hipError_t launch_curve_cp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    const int bw = ocx_block_waves(L->G);
    hipLaunchKernelGGL((ocx_alg_curve_kernel<C, P, CH, nb_for(C, P)>), ocx_grid(L->G, bw),
                       dim3(64 * bw), 0, st, a);
    return hipGetLastError();
}

template <int C, int P, bool CH>
hipError_t launch_comp_cp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    const int64_t n = L->G * a.K;
    const int bw = ocx_block_waves(n);
    hipLaunchKernelGGL((ocx_curve_comp_kernel<C, P, CH, nb_for(C, P)>), ocx_grid(n, bw),
                       dim3(64 * bw), 0, st, a);
    return hipGetLastError();
}

template <int C, int P>
hipError_t launch_pipe_curve_cp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    constexpr int NB = pipe_nb<C>(P);
    constexpr bool RT = pipe_rt<C, P, 1>();
    const int bw = pipe_block_waves(L->G);
    const dim3 grid = ocx_grid(L->G, bw), block(64 * bw);
    if (a.ftl)
        hipLaunchKernelGGL((ocx_alg_pipe_curve_kernel<C, P, NB, true, RT>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((ocx_alg_pipe_curve_kernel<C, P, NB, false, RT>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pipe_curve(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    return ocx_pipe_dispatch(L, [&](auto c, auto p) {
        return launch_pipe_curve_cp<decltype(c)::value, decltype(p)::value>(L, a, st);
    });
}

hipError_t launch_plain_curve(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    OCX_DISPATCH(launch_curve_cp, L, a, st)
}

hipError_t launch_curve_comp(const ocx_layout* L, const CurveArgs& a, hipStream_t st) {
    OCX_DISPATCH(launch_comp_cp, L, a, st)
}

}  // namespace

int64_t ocx_curve_ws_bytes(const ocx_layout* L, int64_t K) {
    return L->G * K * 64 * (8 * (int64_t)L->C + 8 + 4);
}

hipError_t ocx_launch_alg_curve(const ocx_layout* L, const double* zt, const double* yt, int ftl,
                                double eta0, const int64_t* ck, int64_t K, double* reg,
                                double* cum, double* comp, int* closed_out, int onepass,
                                void* ws, hipStream_t st) {
    if (L->G == 0 || K <= 0) return hipSuccess;
    CurveArgs a{};
    a.p.zt = zt;
    a.p.yt = yt;
    a.p.B = L->B;
    a.p.T = L->T;
    a.p.G = L->G;
    a.p.eta0 = eta0;
    a.p.regret = reg;
    a.p.cum_out = cum;
    a.p.comp_out = comp;
    a.p.closed_out = closed_out;
    a.p.onepass = onepass;
    a.p.gn = L->G;  // every group, the whole horizon
    a.p.tn = L->T;
    a.ftl = ftl;
    a.ck = ck;
    a.K = K;
    const int64_t slots = L->G * K * 64;
    a.ws_theta = static_cast<double*>(ws);
    a.ws_cum = a.ws_theta + slots * L->C;
    a.ws_need = reinterpret_cast<int*>(a.ws_cum + slots);
    hipError_t e = ocx_alg_use_pipe(L) ? launch_pipe_curve(L, a, st) : launch_plain_curve(L, a, st);
    if (e != hipSuccess) return e;
    return launch_curve_comp(L, a, st);
}
