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
#include <map>
#include <mutex>

#include "ocx_alg_pipe.h"
#include "ocx_device_math.h"
#include "ocx_internal.h"
#include "ocx_sim_kernels.h"

// BITS: the instances that read the label-bit tile (ocx_alg_pipe.h) — the persistent 8 x 8
// instance, FTRL and FTL: what a resident d = 64 batch of more groups than one round holds
// launches (the bench).  Every other launch keeps y_tiled: the full 8 x 8 form measured slower
// from bits on the few-wave batches (4 900 x 1e5 x 64: 39.8 -> 45.5 ms; a latency-bound wave
// pays for the block-boundary word load), and the lean and chunked forms run beside a
// generator that would pay more for writing the tile than the pass saves (DESIGN.md §3.1,
// §3.2).  Resource reports: profiles/label_bits_resources.txt.
template <int C, int P, int NB, bool FTL, int MINW = 1, bool CHUNK = false, bool LOOP = false,
          bool BITS = false>
__global__ __launch_bounds__(OCX_BLOCK, MINW) void ocx_alg_pipe_kernel(PipeArgs a) {
    alg_pipe_body<C, P, NB, FTL, pipe_rt<C, P, MINW>(), CHUNK, PipeNoObserver, LOOP, BITS>(a);
}

// OCX_LABEL_BITS=0: every launch reads y_tiled's doubles (A/B inside one build)
static bool label_bits_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("OCX_LABEL_BITS");
        return !e || std::atoi(e) != 0;
    }();
    return on;
}

// ---------------------------------------------------------------------------
// The persistent launch: a batch of more groups than are resident at once
// ---------------------------------------------------------------------------
// The full form compiles to 212 VGPRs at 8 x 8 (two waves per SIMD), so a launch of more
// than 2 x 4 x CUs groups runs in dispatcher rounds, each wave with NB − 2 steps of loads in
// flight: 4 096 groups are two rounds of 2 048 waves x 7 steps, ≈60 MB outstanding where
// latency x bandwidth needs ≈8.6 MB.  Such a batch instead launches OCX_PIPE_PERS_WPS waves
// per SIMD of an instance with a ring of OCX_PIPE_PERS_NB slots, once, and every wave loops
// over its share of the groups (alg_pipe_body, LOOP).  Four-wave blocks, one wave per SIMD;
// where the instance's registers admit more blocks per CU than wanted, a dynamic-LDS request
// the kernel never touches caps them, so no CU takes two blocks while another takes none.
// Measured at the bench batch (profiles/persistent_sweep.jsonl): what counts
// is the residency — one wave per SIMD 26.06–26.13 ms at every ring depth tried (2, 3, 4, 7
// steps in flight), two per SIMD 26.41–26.45 ms, the two-round launch 26.48–26.51 ms — so the
// shipped point is one wave per SIMD with the shortest ring.  Under a 128-VGPR budget
// (MINW = 4) the looped form spills (24 B per lane at 4 slots), so the instance takes the
// 256-VGPR budget: 132 VGPRs, no scratch.  8 x 8 only: the layout of the d = 64 batches
// large enough to get here; FTRL and FTL alike (25.94 -> 25.32 ms for FTL,
// profiles/persistent_pipe_lib_ab.jsonl).
#ifndef OCX_PIPE_PERS_NB
#define OCX_PIPE_PERS_NB 4
#endif
#ifndef OCX_PIPE_PERS_MINW  // the instance's register budget: 512 / MINW VGPRs
#define OCX_PIPE_PERS_MINW 2
#endif
#ifndef OCX_PIPE_PERS_WPS
#define OCX_PIPE_PERS_WPS 1
#endif
#ifndef OCX_PIPE_PERS_TUNE  // tuning builds (tools/persistent_sweep.py): the launch shape from
#define OCX_PIPE_PERS_TUNE 0  // OCX_PIPE_PERS_WPS / OCX_PIPE_PERS_BW in the environment, per launch
#endif

template <int C, int P>
constexpr bool pipe_persistent_layout() {
    return C == 8 && P == 8;
}

namespace {
struct PersGeom {
    hipError_t err = hipSuccess;
    int64_t round = 0;  // waves of the one-group-per-wave instance resident at once
    int64_t nw = 0;     // waves the persistent launch starts
    size_t lds = 0;     // its dynamic-LDS request (the cap on blocks per CU)
};

// Blocks of bw waves per CU so that `wps` waves sit on each SIMD, and the LDS request that
// keeps the dispatcher to that many.
template <class K>
hipError_t pers_shape(K kern, int dev, int cus, int wps, int bw, PersGeom& gm) {
    const int want = wps * 4 / bw;
    int lds_cu = 0, q = 0;
    if (hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) !=
            hipSuccess || lds_cu <= 0)
        lds_cu = 160 * 1024;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kern, 64 * bw, 0);
    if (e != hipSuccess) return e;
    size_t lds = 0;
    if (q > want) {
        for (lds = ((size_t)lds_cu / (want + 1) / 512 + 1) * 512; lds <= (size_t)lds_cu; lds += 512) {
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kern, 64 * bw, lds);
            if (e != hipSuccess) return e;
            if (q <= want) break;
        }
    }
    if (q <= 0 || q > want) return hipErrorInvalidConfiguration;
    gm.lds = lds;
    gm.nw = (int64_t)q * bw * cus;
    return hipSuccess;
}

template <int C, int P>
PersGeom pers_geometry(int ftl, bool bits) {
    constexpr int NB = pipe_nb<C>(P), NBP = OCX_PIPE_PERS_NB, MW = OCX_PIPE_PERS_MINW;
    PersGeom gm;
    int dev = 0, cus = 0;
    if ((gm.err = hipGetDevice(&dev)) != hipSuccess) return gm;
    int wps = OCX_PIPE_PERS_WPS, bw = 4;
#if OCX_PIPE_PERS_TUNE
    if (const char* e = std::getenv("OCX_PIPE_PERS_WPS")) wps = std::atoi(e);
    if (const char* e = std::getenv("OCX_PIPE_PERS_BW")) bw = std::atoi(e);
    if (wps < 1 || wps > 8 || (bw != 1 && bw != 4)) return gm.err = hipErrorInvalidValue, gm;
#else
    static std::mutex mu;
    static std::map<std::pair<int, int>, PersGeom> cache;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(dev, (ftl ? 1 : 0) | (bits ? 2 : 0));
    const auto it = cache.find(key);
    if (it != cache.end()) return it->second;
#endif
    if ((gm.err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess)
        return gm;
    int q = 0;
    gm.err = ftl ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, ocx_alg_pipe_kernel<C, P, NB, true>, 256, 0)
                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, ocx_alg_pipe_kernel<C, P, NB, false>, 256, 0);
    if (gm.err != hipSuccess) return gm;
    gm.round = (int64_t)q * 4 * cus;
    // (round: the float64 form's in both cases, so the labels' form never moves the policy)
    if (bits)
        gm.err = ftl ? pers_shape(ocx_alg_pipe_kernel<C, P, NBP, true, MW, false, true, true>, dev, cus, wps, bw, gm)
                     : pers_shape(ocx_alg_pipe_kernel<C, P, NBP, false, MW, false, true, true>, dev, cus, wps, bw, gm);
    else
        gm.err = ftl ? pers_shape(ocx_alg_pipe_kernel<C, P, NBP, true, MW, false, true>, dev, cus, wps, bw, gm)
                     : pers_shape(ocx_alg_pipe_kernel<C, P, NBP, false, MW, false, true>, dev, cus, wps, bw, gm);
#if !OCX_PIPE_PERS_TUNE
    if (gm.err == hipSuccess) cache.emplace(key, gm);
#endif
    return gm;
}

// nwaves > 0 (ocx_test_alg_pipe_persistent): that many waves instead of the geometry's
template <int C, int P>
hipError_t launch_pipe_persistent(PipeArgs a, int ftl, int64_t nwaves, const PersGeom& gm,
                                  hipStream_t st) {
    constexpr int NBP = OCX_PIPE_PERS_NB, MW = OCX_PIPE_PERS_MINW;
    int bw = 4;
#if OCX_PIPE_PERS_TUNE
    if (const char* e = std::getenv("OCX_PIPE_PERS_BW")) bw = std::atoi(e) == 1 ? 1 : 4;
#endif
    a.gstride = nwaves > 0 ? nwaves : gm.nw;
    const dim3 grid = ocx_grid(a.gstride, bw), block(64 * bw);
    if (a.yb && ftl)
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<C, P, NBP, true, MW, false, true, true>), grid, block, gm.lds, st, a);
    else if (a.yb)
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<C, P, NBP, false, MW, false, true, true>), grid, block, gm.lds, st, a);
    else if (ftl)
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<C, P, NBP, true, MW, false, true>), grid, block, gm.lds, st, a);
    else
        hipLaunchKernelGGL((ocx_alg_pipe_kernel<C, P, NBP, false, MW, false, true>), grid, block, gm.lds, st, a);
    return hipGetLastError();
}

template <int C, int P>
hipError_t launch_pipe_cp(const PipeArgs& a, int ftl, hipStream_t st) {
    constexpr int NB = pipe_nb<C>(P);
    if constexpr (pipe_persistent_layout<C, P>()) {
        // more groups than one round holds; every smaller batch (the few-wave T = 1e5 shapes,
        // the capacity-limited ones) keeps its one-group-per-wave launch below
        if (!a.state) {
            const PersGeom gm = pers_geometry<C, P>(ftl, a.yb != nullptr);
            if (gm.err != hipSuccess) return gm.err;
            if (a.gn > gm.round) return launch_pipe_persistent<C, P>(a, ftl, 0, gm, st);
        }
    }
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

PipeArgs pipe_args(const ocx_layout* L, const double* zt, const double* yt, const uint64_t* yb,
                   double eta0, double* reg, double* cum, double* comp, int* closed_out,
                   int onepass) {
    PipeArgs a{};
    a.zt = zt;
    a.yt = yt;
    a.yb = label_bits_enabled() ? yb : nullptr;
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
    a.gstride = L->G;
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
                               int* closed_out, int onepass, hipStream_t st, const uint64_t* yb) {
    if (L->G == 0) return hipSuccess;
    return launch_pipe(L, pipe_args(L, zt, yt, yb, eta0, reg, cum, comp, closed_out, onepass), ftl, st);
}

bool ocx_pipe_persistent_supported(const ocx_layout* L) {
    return ocx_pipe_supported(L) && L->C == 8 && L->P == 8;
}

// The persistent instance with `nwaves` waves, whatever the batch's size (the policy above
// takes it only past one round): ocx_test_alg_pipe_persistent.
hipError_t ocx_launch_alg_pipe_persistent(const ocx_layout* L, const double* zt, const double* yt,
                                          int ftl, double eta0, double* reg, double* cum,
                                          double* comp, int* closed_out, int onepass,
                                          int64_t nwaves, hipStream_t st, const uint64_t* yb) {
    if (!ocx_pipe_persistent_supported(L) || nwaves <= 0) return hipErrorInvalidValue;
    if (L->G == 0) return hipSuccess;
    const PipeArgs a = pipe_args(L, zt, yt, yb, eta0, reg, cum, comp, closed_out, onepass);
    const PersGeom gm = pers_geometry<8, 8>(ftl, a.yb != nullptr);
    if (gm.err != hipSuccess) return gm.err;
    return launch_pipe_persistent<8, 8>(a, ftl, nwaves, gm, st);
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
    PipeArgs a = pipe_args(L, zt, yt, nullptr, eta0, reg, nullptr, nullptr, nullptr, onepass);
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
    PipeArgs a = pipe_args(L, zt, yt, nullptr, eta0, reg, nullptr, nullptr, nullptr, onepass);
    a.t0 = t0;
    a.tn = tn;
    a.state = state;
    a.bad = bad;
    a.gmax = t0 + tn >= L->T ? gmax : nullptr;  // the chunk that writes the regrets
    return ocx_pipe_lean_supported(L) ? launch_lean(L, a, st) : launch_pipe(L, a, 0, st);
}
