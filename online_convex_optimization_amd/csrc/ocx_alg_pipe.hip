// ocx_alg_pipe.hip — FTRL/FTL (fast_algorithms.py:88-115) for the butterfly-sum layouts
// (P >= 2 lanes per sequence, chain = 0) with the step's dependency chain cut short.
//
// In the plain kernel (ocx_sim.hip) step t waits for g_{t-1}, then forms x = sθ_t, sums
// ||x||² and z_t·x lane by lane (C dependent adds each), crosses the P lanes, and — when
// the FTRL action is rescaled — sums z_t·x a second time: about 60 dependent fp64
// operations, ≈1 100 cycles per step.  A few-wave batch (capacity-limited long horizons:
// d = 64, T = 1e5, ≈4 900 sequences, one wave per SIMD) cannot hide that, so its time is
// T × that latency.
//
// Here every lane-local product of step t is formed BEFORE g_{t-1} is known, from the
// lagging state θ' = θ_{t-1} (θ_t = θ' + g_{t-1} z_{t-1}):
//     A = z_t·θ',  Bz = z_t·z_{t-1},  U = θ'·θ',  V = θ'·z_{t-1},  W = z_{t-1}·z_{t-1}
// (per lane, over its C coordinates), so that once g = g_{t-1} arrives
//     z_t·θ_t = A + g·Bz,   ||θ_t||² = U + g·(2V + g·W)
// are one or two fma per lane, then the P-lane butterflies; FTRL's action follows as
//     s_abs = |s_t|·sqrt(||θ_t||²),  f = 1/s_abs if s_abs > 1 else 1,  q = (s_t·(z_t·θ_t))·f
// and FTL's as q = (−1/sqrt(||θ_t||²))·(z_t·θ_t) (0 when θ_t = 0).  The chain is ≈25
// dependent operations; the C-wide products run beside it.  θ itself is updated exactly
// as the reference does (θ += g·z, g a power of two), so the trajectory is the
// reference's; each step's q carries the butterfly layouts' usual ~1e-16 relative
// rounding difference (tests/test_gpu_parity.py: 1e-12 bar).  For rows with a single
// nonzero coordinate (the flip / switching families, exact ties) every quantity above
// is exact and equal to the reference's (sqrt of an exact square is exact; s_abs =
// |fl(s θ_j)| and f = fl(1/s_abs) then reproduce the reference's rescale bit for bit).
// FTL near θ = 0, where ||θ_t||² = U + g(2V + gW) would lose relative accuracy to
// cancellation, re-sums ||θ_t||² directly (||θ_t||² < 0.25: early steps, returns to the
// origin).  The comparator pass / closed form are those of ocx_alg_kernel.
//
// Chunked runs (the trailing pipeline, ocx_pipeline.hip): a launch may cover steps
// [t0, t0 + tn) of the horizon only (t0 a multiple of 64), carrying the step's whole state —
// θ_{t-1}, z_{t-1}, the lane partials A, Bz, V, W, g_{t-1}, the loss and the `clean` flag —
// through HBM between launches.  U and the FTRL scales are re-formed at the chunk's first
// step (a multiple of 64: their periodic refresh), so a chunked run is the whole run, bit for
// bit.  The rows before t0 may already hold the next batch, so a chunked run never streams
// the second comparator pass: a sequence the closed form cannot certify gets a NaN regret
// and raises *bad (the caller runs its batch again in the sequential path).
#include <cmath>

#include "ocx_alg_pipe.h"
#include "ocx_device_math.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

template <int C, int P, int NB, bool FTL, int MINW = 1, bool CHUNK = false>
__global__ __launch_bounds__(OCX_BLOCK, MINW) void ocx_alg_pipe_kernel(PipeArgs a) {
    alg_pipe_body<C, P, NB, FTL, pipe_rt<C, P, MINW>(), CHUNK>(a);
}

namespace {
template <int C, int P>
hipError_t launch_pipe_cp(const PipeArgs& a, int ftl, hipStream_t st) {
    constexpr int NB = pipe_nb<C>(P);
    const int bw = pipe_block_waves(a.gn);
    const dim3 grid = ocx_grid(a.gn, bw), block(64 * bw);
    if (a.state)  // a chunked run (FTRL: the trailing pipeline's algorithm)
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<C, P, NB, false, 1, true>), grid, block, 0, st, a);
    else if (ftl)
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<C, P, NB, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<C, P, NB, false>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pipe(const ocx_layout* L, const PipeArgs& a, int ftl, hipStream_t st) {
    if (a.gn <= 0) return hipSuccess;
    return ocx_pipe_dispatch(L, [&](auto c, auto p) {
        return launch_pipe_cp<decltype(c)::value, decltype(p)::value>(a, ftl, st);
    });
}

PipeArgs pipe_args(const ocx_layout* L, const double* zt, const double* yt, double eta0,
                   double* reg, double* cum, double* comp, int* closed_out, int onepass) {
    PipeArgs a{};
    a.zt = zt;
    a.yt = yt;
    a.B = L->B;
    a.T = L->T;
    a.G = L->G;
    a.eta0 = eta0;
    a.regret = reg;
    a.cum_out = cum;
    a.comp_out = comp;
    a.closed_out = closed_out;
    a.onepass = onepass;
    a.g0 = 0;
    a.gn = L->G;
    a.t0 = 0;
    a.tn = L->T;
    return a;
}
}  // namespace

bool ocx_pipe_supported(const ocx_layout* L) {
    // T < 2^30: the step counter is a 32-bit int (ocx_ring_loop<..., int>)
    return !L->chain && L->T < ((int64_t)1 << 30) && pipe_layout(L->C, L->P);
}

hipError_t ocx_launch_alg_pipe(const ocx_layout* L, const double* zt, const double* yt, int ftl,
                               double eta0, double* reg, double* cum, double* comp,
                               int* closed_out, int onepass, hipStream_t st) {
    if (L->G == 0) return hipSuccess;
    return launch_pipe(L, pipe_args(L, zt, yt, eta0, reg, cum, comp, closed_out, onepass), ftl, st);
}

int64_t ocx_pipe_state_doubles(const ocx_layout* L) {
    return L->G * 64 * (int64_t)pipe_state_words(L->C);
}

// The lean form (ocx_pipeline.hip: the FTRL side of both pipelines): at most 128 VGPRs, so
// one wave fits on a SIMD beside four generator waves of the 96-VGPR form (the sub-batch
// pipeline) or four of the 80-VGPR few-stream form (the trailing pipeline); a shorter ring
// (OCX_PIPE_LEAN_NB8 / _NB4 slots at 8 / 4 coordinates per lane) is what makes it fit.  FTRL
// only, the pipelines' algorithm; 8 x 8 and 16 x 4 layouts.  One-wave blocks: the dispatcher
// spreads them over the SIMDs the generator leaves room on.
#ifndef OCX_PIPE_LEAN_NB8
#define OCX_PIPE_LEAN_NB8 4
#endif
#ifndef OCX_PIPE_LEAN_NB4
#define OCX_PIPE_LEAN_NB4 8
#endif
bool ocx_pipe_lean_supported(const ocx_layout* L) {
    return !L->chain && L->T < ((int64_t)1 << 30) && ((L->P == 8 && L->C == 8) || (L->P == 16 && L->C == 4));
}

// The layouts the lean form is built for beyond the trailing pipeline's: 8 x 4 (d = 32's
// g(T) layout in the sub-batch pipeline, round 6).
bool ocx_pipe_lean_launchable(const ocx_layout* L) {
    return ocx_pipe_lean_supported(L) || (!L->chain && L->T < ((int64_t)1 << 30) && L->P == 8 && L->C == 4);
}

namespace {
hipError_t launch_lean(const ocx_layout* L, const PipeArgs& a, hipStream_t st) {
    const dim3 grid = ocx_grid(a.gn, 1), block(64);
    if (L->P == 8 && L->C == 4 && !a.state) {
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<4, 8, OCX_PIPE_LEAN_NB4, false, 4>), grid, block, 0, st, a);
    } else if (L->P == 8 && L->C == 8) {
        if (a.state)
            hipLaunchKernelGGL((ocx_alg_pipe_kernel<8, 8, OCX_PIPE_LEAN_NB8, false, 4, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((ocx_alg_pipe_kernel<8, 8, OCX_PIPE_LEAN_NB8, false, 4>), grid, block, 0, st, a);
    } else if (L->P == 16 && L->C == 4) {
        if (a.state)
            hipLaunchKernelGGL((ocx_alg_pipe_kernel<4, 16, OCX_PIPE_LEAN_NB4, false, 4, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((ocx_alg_pipe_kernel<4, 16, OCX_PIPE_LEAN_NB4, false, 4>), grid, block, 0, st, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
}  // namespace

hipError_t ocx_launch_alg_pipe_lean(const ocx_layout* L, const double* zt, const double* yt,
                                    double eta0, double* reg, int onepass, int64_t g0,
                                    int64_t gn, unsigned long long* gmax, hipStream_t st) {
    if (gn <= 0) return hipSuccess;
    if (g0 < 0 || g0 + gn > L->G) return hipErrorInvalidValue;
    PipeArgs a = pipe_args(L, zt, yt, eta0, reg, nullptr, nullptr, nullptr, onepass);
    a.g0 = g0;
    a.gn = gn;
    a.gmax = gmax;
    return launch_lean(L, a, st);
}

// Chunked runs take the lean form where the layout has one (the trailing pipeline's
// layouts: it runs beside the generator), the full form otherwise (tests of other layouts).
hipError_t ocx_launch_alg_pipe_chunk(const ocx_layout* L, const double* zt, const double* yt,
                                     double eta0, double* reg, int onepass, int64_t t0,
                                     int64_t tn, double* state, int* bad,
                                     unsigned long long* gmax, hipStream_t st) {
    if (L->G == 0 || tn <= 0) return hipSuccess;
    // onepass only: a chunk after the first cannot stream the second comparator pass
    if (t0 < 0 || t0 % 64 != 0 || t0 + tn > L->T || !state || !onepass || !ocx_pipe_supported(L))
        return hipErrorInvalidValue;
    PipeArgs a = pipe_args(L, zt, yt, eta0, reg, nullptr, nullptr, nullptr, onepass);
    a.t0 = t0;
    a.tn = tn;
    a.state = state;
    a.bad = bad;
    a.gmax = t0 + tn >= L->T ? gmax : nullptr;  // the chunk that writes the regrets
    return ocx_pipe_lean_supported(L) ? launch_lean(L, a, st) : launch_pipe(L, a, 0, st);
}
