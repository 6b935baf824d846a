// ocx_alg_pipe.h — the pipelined FTRL/FTL loop (ocx_alg_pipe.hip describes the step) and its
// launch policy.  The loop is ocx_alg_pipe_kernel's and, with a per-step observer, its curve
// form's (ocx_alg_curve.hip).  The step-size form (ocx_alg_etas.hip) keeps its own written-out
// loop and shares the launch policy and ocx_pipe_wave_id only.
#pragma once
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "ocx_alg_step.h"
#include "ocx_sim_kernels.h"

// The step counter's type (ocx_ring_loop): int keeps the loop tests on the scalar unit; used
// for C <= OCX_PIPE_IT32_MAXC coordinates per lane.  Measured (r04_pipe_ab1.jsonl): the 16 x 4
// few-wave batch 35.5 -> 32.4 ms with it, while the 8 x 8 kernel's loads were scheduled with
// shallower waits and it ran 40.2 -> 42.0 ms, so 8 x 8 keeps the int64_t counter.
#ifndef OCX_PIPE_IT32_MAXC
#define OCX_PIPE_IT32_MAXC 4
#endif
template <int C>
using pipe_step_t = typename std::conditional<(C <= OCX_PIPE_IT32_MAXC), int, int64_t>::type;

// Per-lane state words of a chunked run (ocx_alg_pipe.hip): θ_{t-1} [C], z_{t-1} [C], then
// A, Bz, V, W, g_{t-1}, cum, clean.  Stored word-major per wave-group: word i of lane l of
// group g at state[(g·NS + i)·64 + l], so each word is one coalesced 512-B access.
constexpr int pipe_state_words(int C) { return 2 * C + 7; }

// Wave-group of this wave when gn groups run in blocks of W waves.  A plain blockIdx * W +
// wave mapping leaves the nblk * W − gn spare slots in the last block, so a few-wave launch
// ends with a block of one or two waves, alone on its CU — and a lone FTL wave measured
// ≈10 % slower than its neighbours in full blocks, setting the launch's time
// (profiles/r04_wave_clock*.jsonl).  Here the last `idle` blocks hold W − 1 groups each
// instead (W = 4: at least three waves per CU); a spare slot gets gn and exits.
__device__ __forceinline__ int64_t ocx_pipe_wave_id(int64_t gn) {
    const int64_t W = blockDim.x >> 6, blk = blockIdx.x, w = threadIdx.x >> 6;
    const int64_t idle = (int64_t)gridDim.x * W - gn;
    const int64_t full = (int64_t)gridDim.x - idle;  // blocks of W groups
    if (idle <= 0 || full < 0 || blk < full) return blk * W + w;
    return w < W - 1 ? full * W + (blk - full) * (W - 1) + w : gn;
}

// Launch arguments of the loop (one struct: the launchers forward it unchanged).
struct PipeArgs {
    const double* zt;
    const double* yt;
    int64_t B, T, G;
    double eta0;
    double* regret;
    double* cum_out;
    double* comp_out;
    int* closed_out;
    int onepass;
    int64_t g0, gn;  // wave-groups [g0, g0 + gn) of the layout
    int64_t gstride; // persistent launches (alg_pipe_body, LOOP): the waves launched
    int64_t t0, tn;  // steps [t0, t0 + tn) (a whole run: 0, T)
    double* state;   // chunked runs: the carried state (nullable: whole run)
    int* bad;        // chunked runs: set when a sequence needs the second pass
    unsigned long long* gmax;  // nullable: g(T) = max(0, max regret) folded in (bit pattern)
    // nullable: the label-bit tile (BITS instances read it instead of yt).  Last, so that every
    // other field keeps its kernel-argument offset and the float64 instances their code.
    const uint64_t* yb;
};

#ifndef OCX_PIPE_WAVE_CLOCK  // diagnostic build: per-wave clocks instead of cum / comp (below)
#define OCX_PIPE_WAVE_CLOCK 0
#endif

// No observer: the loop and the epilogue of ocx_alg_pipe_kernel, nothing else compiled in.
struct PipeNoObserver {};

// The loop, then the epilogue.  With an observer (the curve form, ocx_alg_curve.hip):
// obs.step(t, …) at every step once th holds θ_t, while cum and clean cover the steps before
// t, and obs.finish(…) with θ_T in place of the epilogue below.  Both calls are compiled in
// only where there is an observer: an empty inlined call is not free (it moved registers and
// scratch in the lean forms).
// RT (FTRL): the rescale's sqrt only in waves where a sequence may need the rescale (see the
// step).  CHUNK: a chunked run (t0, tn, state); the whole-run kernels compile without it, so
// its bookkeeping costs them no registers (the lean form spilled with it: 148 B per lane).
// One wave-group's run: group wv (wave-uniform) of the launch's gn.  Every piece of state is
// local to the call, so a wave that runs several groups (alg_pipe_body, LOOP) starts each from
// scratch: the ring is filled again (one load latency per group) and nothing is carried over.
// BITS: the labels come from the label-bit tile (include/ocx.h: one 64-bit word per sequence
// and 64-step block, bit t mod 64 set where y_t = +1) instead of y_tiled's doubles: no label
// load and no label ring slot per step; the lane loads its sequence's word one block ahead
// (clamped at the horizon's last block, as the look-ahead is) and forms y_t = ±1.0 from bit
// t mod 64 with a wave-uniform shift.  The same doubles reach the same arithmetic, so the
// results are the float64 path's bit for bit wherever every label of a real sequence is ±1.
// A padding sequence (b >= B) differs inside the wave: its bits are 0, so it runs with y = −1.0
// where y_tiled gives it 0.0, and with its all-zero rows it stays `clean`.  Nothing of it gets
// out: every vote and output is gated on `live` (closed = onepass && (clean || !live), so it
// never asks for the second pass on either path; gmax, regret, cum, comp, closed_out are
// written for live sequences only), and θ stays 0 either way (g·z = 0).
template <int C, int P, int NB, bool FTL, bool RT, bool CHUNK, class Obs, bool BITS = false>
__device__ __forceinline__ void alg_pipe_group(const PipeArgs& a, const int64_t wv, Obs& obs) {
    static_assert(P >= 2 && NB >= 4, "butterfly layouts, a ring holding z_{t-1} .. z_{t+1}");
    constexpr bool OBS = !std::is_same<typename std::decay<Obs>::type, PipeNoObserver>::value;
    using IT = pipe_step_t<C>;
    constexpr int S = 64 / P;
    constexpr int K = C / 2;
    constexpr int NS = pipe_state_words(C);
    const int lane = threadIdx.x & 63;
    const int64_t g = a.g0 + wv;
    const int64_t T = a.T, t0 = CHUNK ? a.t0 : 0, tn = CHUNK ? a.tn : T;
    const bool first = !CHUNK || t0 == 0, last = !CHUNK || t0 + tn >= T;
    const double eta0 = a.eta0;
#if OCX_PIPE_WAVE_CLOCK  // diagnostic build only: see the end of the body
    const uint64_t clk0 = __builtin_amdgcn_s_memrealtime();
#endif
    const int s = lane / P;
    const int c = lane % P;
    const int64_t b = g * S + s;
    // The layout's padding sequences (b >= B, the last wave-group's spare slots) have all-zero
    // rows, so their θ stays 0 and FTL's near-origin re-sum would run for them at every step —
    // in the one wave that holds them, which then set the launch's time (a 47.6 ms straggler
    // among 41–42 ms waves on the 4 900 x 1e5 batch, profiles/r04_wave_clock*.jsonl).  Their
    // results are never written, so they skip it.
    const bool live = b < a.B;
    const int64_t tstride = 64;  // ocx_d2 per step within a plane
    const ocx_d2* __restrict__ zg = reinterpret_cast<const ocx_d2*>(a.zt) + (g * T + t0) * tstride;
    const int64_t kst = a.G * T * 64;  // plane stride (pairs k)
    const double* __restrict__ yg = a.yt + (g * T + t0) * S;
    // BITS: this lane's word of block kb at ybg[kb * S]; KB blocks in the horizon
    const int64_t KB = (T + 63) >> 6;
    const uint64_t* __restrict__ ybg = BITS ? a.yb + g * KB * S + s : nullptr;
    auto ybit = [](uint64_t w, int sh) -> double {  // bit sh of w: 1 -> +1.0, 0 -> -1.0
        return __hiloint2double((int)(0xBFF00000u ^ ((uint32_t)(w >> sh) << 31)), 0);
    };
    // word i of this lane's carried state (formed where used: nothing stays live over the loop)
    auto stw = [&](int i) -> double& { return a.state[(g * NS + i) * 64 + lane]; };

    double th[C];  // θ_{t-1} (lagging one update)
    double gp = 0.0;                                   // g_{t-1}
    double A = 0.0, Bz = 0.0, U = 0.0, V = 0.0, W = 0.0;  // step t's lane partials
    double cum = 0.0;
    bool clean = true;  // onepass: rows in the ball, every sub-gradient −y_t/2
    // z_{t-1} is read where it lies, in the slot before step t's: the late loads
    // (ocx_ring_loop<NB, true>) refill that slot only after step t.  At t = 0 that slot is
    // zero (g_{-1} = 0 multiplies it); a later chunk restores z_{t0-1} there.
    ocx_d2 zb[NB][K];
    double yb[BITS ? 1 : NB];
    uint64_t ywc = 0, ywn = 0;  // BITS: the current block's word, the next block's
    if constexpr (BITS) {
        if (tn > 0) ywn = ybg[(t0 >> 6) * S];
    }
    if (first) {
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) zb[NB - 1][k] = ocx_d2{0.0, 0.0};
    } else if constexpr (CHUNK) {
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = stw(j);
#pragma unroll
        for (int k = 0; k < K; ++k) zb[NB - 1][k] = ocx_d2{stw(C + 2 * k), stw(C + 2 * k + 1)};
        A = stw(2 * C);
        Bz = stw(2 * C + 1);
        V = stw(2 * C + 2);
        W = stw(2 * C + 3);
        gp = stw(2 * C + 4);
        cum = stw(2 * C + 5);
        clean = stw(2 * C + 6) != 0.0;
    }
    auto load = [&](int slot, int64_t tl) {
        const ocx_d2* __restrict__ row = zg + tl * tstride;  // uniform
#pragma unroll
        for (int k = 0; k < K; ++k) {
#if OCX_LOAD_NT
            zb[slot][k] = __builtin_nontemporal_load(row + k * kst + lane);
#else
            zb[slot][k] = row[k * kst + lane];
#endif
        }
        if constexpr (!BITS) yb[slot] = yg[tl * S + s];
    };

    double scv = 0.0;  // −η0/√(t+1+lane) for the 64 steps from the last multiple of 64

    ocx_ring_loop<NB, true, IT>(tn, load, [&](int u, int64_t tl) {
        const int64_t t = t0 + tl;
        if ((tl & 63) == 0) {
            ocx_pipe_refresh<FTL>(t, lane, eta0, scv, th, U);
            if constexpr (BITS) {
                const int64_t kn = (t >> 6) + 1;
                ywc = ywn;
                ywn = ybg[(kn < KB ? kn : KB - 1) * S];
            }
        }
        // ---- chain: g_{t-1} → z_t·θ_t, ||θ_t||² → q_t → g_t
        const double zth = __builtin_fma(gp, Bz, A);
        double tth = __builtin_fma(gp, __builtin_fma(gp, W, 2.0 * V), U);
        const ocx_d2* zp1 = zb[(u + NB - 1) % NB];
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = __builtin_fma(gp, ocx_zj(zp1, j), th[j]);
        if constexpr (OBS) obs.step(t, g, b, c, lane, live, th, cum, clean);
        const double q_raw = ocx_seq_sum<P>(zth);
        double n_raw = ocx_seq_sum<P>(tth);
        double qt;
        if constexpr (!FTL)
            qt = ocx_pipe_q_ftrl<RT>(ocx_readlane(scv, (int)(tl & 63)), q_raw, n_raw);
        else
            qt = ocx_pipe_q_ftl<C, P>(th, q_raw, n_raw, tth, live);
        const double yv = BITS ? ybit(ywc, (int)(tl & 63)) : yb[u];
        const double gq = ocx_loss_grad(qt, yv, cum);
        ocx_cert_grad<BITS>(clean, yv, gq);
        // ---- off the chain; z_{t+1} is in flight since NB-2 steps
        ocx_pipe_advance<P>(th, zb[u], zb[(u + 1) % NB], a.onepass, zth, tth, gq, A, Bz, U, V, W, gp,
                            clean);
    }, CHUNK ? T - t0 : T);
    // the chunk's last row: z_{t1-1} for the next chunk, or z_{T-1} for θ_T (loaded again:
    // its ring slot is not known at compile time)
    ocx_d2 zl[K];
    if (tn > 0) ocx_load_tile<C>(zl, zg + (tn - 1) * tstride + lane, kst);
    if constexpr (CHUNK) if (!last) {
#pragma unroll
        for (int j = 0; j < C; ++j) stw(j) = th[j];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            stw(C + 2 * k) = zl[k].x;
            stw(C + 2 * k + 1) = zl[k].y;
        }
        stw(2 * C) = A;
        stw(2 * C + 1) = Bz;
        stw(2 * C + 2) = V;
        stw(2 * C + 3) = W;
        stw(2 * C + 4) = gp;
        stw(2 * C + 5) = cum;
        stw(2 * C + 6) = clean ? 1.0 : 0.0;
        return;
    }
    if (tn > 0) {
#pragma unroll
        for (int j = 0; j < C; ++j) th[j] = __builtin_fma(gp, ocx_zj(zl, j), th[j]);
    }
    if constexpr (OBS) {
        obs.finish(g, b, c, lane, live, th, cum, clean);
        return;
    }

    // ---- comparator: closed form where certified (ocx_alg_kernel onepass), else the
    // reference's second streaming pass with x* = FTL(θ_T) (fast_algorithms.py:113-114) —
    // which a chunked run (t0 > 0: the early rows may hold the next batch) cannot stream
    const bool closed = a.onepass && (clean || !live);
    double comp = 0.0;
    if (__ballot(!closed) != 0) {  // wave-uniform
        if (first) {  // zg, yg: row 0
            double xs[C];
            ocx_action_ftl<C, P, false>(th, xs, lane);
            if constexpr (BITS) {
                if (T > 0) ywn = ybg[0];  // (T = 0: the tile has no word)
            }
            ocx_ring_loop<NB, false, IT>(T, load, [&](int u, int64_t tl) {
                if constexpr (BITS) {
                    if ((tl & 63) == 0) {
                        const int64_t kn = (tl >> 6) + 1;
                        ywc = ywn;
                        ywn = ybg[(kn < KB ? kn : KB - 1) * S];
                    }
                }
                double p[C];
#pragma unroll
                for (int j = 0; j < C; ++j) p[j] = ocx_zj(zb[u], j) * xs[j];
                const double qq = ocx_total<C, P, false>(p, lane);
                comp += 0.5 * fabs(qq - (BITS ? ybit(ywc, (int)(tl & 63)) : yb[u]));
            });
        } else if constexpr (CHUNK) {
            comp = __builtin_nan("");
            if (!closed && c == 0 && a.bad) *a.bad = 1;
        }
    }
    if (__ballot(closed) != 0) {
        double p[C];
#pragma unroll
        for (int j = 0; j < C; ++j) p[j] = th[j] * th[j];
        const double nrm = sqrt(ocx_total<C, P, false>(p, lane));
        if (closed) comp = 0.5 * (double)T - nrm;
    }
    // g(T) folded in here (the pipelines' FTRL launches): no separate launch that would wait
    // for a free slot beside the generator (2-3 ms each)
    if (a.gmax && __ballot(live) != 0) {  // wave-uniform
        const double rg = cum - comp;
        double mv = (c == 0 && live && rg > 0.0) ? rg : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double u = __shfl_xor(mv, o, 64);
            if (u > mv) mv = u;
        }
        if (lane == 0 && mv > 0.0) atomicMax(a.gmax, (unsigned long long)__double_as_longlong(mv));
    }
    if (c == 0 && live) {
        if (a.regret) a.regret[b] = cum - comp;
#if OCX_PIPE_WAVE_CLOCK
        // diagnostic build (tools/wave_clock_probe.py): the wave's duration in ticks of the
        // 100 MHz real-time clock, and where it ran (HW_ID, XCC_ID) — not results
        const uint64_t clk1 = __builtin_amdgcn_s_memrealtime();
        if (a.cum_out) a.cum_out[b] = (double)(clk1 - clk0);
        if (a.comp_out) a.comp_out[b] = (double)clk0;
        if (a.closed_out)
            a.closed_out[b] = (int)((__builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xffffu) |
                                    ((__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xfu) << 16));
#else
        if (a.cum_out) a.cum_out[b] = cum;
        if (a.comp_out) a.comp_out[b] = comp;
        if (a.closed_out) a.closed_out[b] = closed ? 1 : 0;
#endif
    }
}

// Which groups a wave runs.  Without LOOP: its one group (ocx_pipe_wave_id; a spare slot
// leaves).  With LOOP (the persistent launch, launch_pipe_cp): wave w of the a.gstride launched
// runs groups w, w + gstride, ... < gn, one after the other — a plain loop, no hand-off between
// waves; a wave beyond gstride (the last block's spare slots) leaves.
template <int C, int P, int NB, bool FTL, bool RT, bool CHUNK = false, class Obs = PipeNoObserver,
          bool LOOP = false, bool BITS = false>
__device__ __forceinline__ void alg_pipe_body(const PipeArgs& a, Obs&& obs = Obs{}) {
    // wave-uniform, provably (readfirstlane): the tile bases live in SGPRs and every load
    // is an SGPR base + the lane's constant offset, with no per-load address arithmetic
    if constexpr (!LOOP) {
        const int64_t wv = (int64_t)__builtin_amdgcn_readfirstlane((int)ocx_pipe_wave_id(a.gn));
        if (wv >= a.gn) return;
        alg_pipe_group<C, P, NB, FTL, RT, CHUNK, Obs, BITS>(a, wv, obs);
    } else {
        static_assert(!CHUNK, "a chunked run carries one group's state per wave");
        const int64_t w0 = (int64_t)__builtin_amdgcn_readfirstlane((int)ocx_wave_id());
        if (w0 >= a.gstride) return;
        for (int64_t wv = w0; wv < a.gn; wv += a.gstride)
            alg_pipe_group<C, P, NB, FTL, RT, CHUNK, Obs, BITS>(a, wv, obs);
    }
}

// ---------------------------------------------------------------------------
// Launch policy of the pipelined kernels (host)
// ---------------------------------------------------------------------------
// The pipelined step pays where one wave's step latency sets the batch time: the few-wave
// butterfly layouts OCX_LANES_BEST chooses (8 x 8, 16 x 4 at d = 64; 16 x 16; 32 x 32 at
// d = 1024) and their neighbours, and 64 x 16 at d = 1024 (lanes_per_seq = 64: 17.4 vs
// 19.2-19.7 ms for the 32 x 32 layout's pass over 2 688 x 5 000 steps,
// profiles/r05_genscale.jsonl).  Other butterfly layouts keep the plain kernel.  This is the
// set ocx_pipe_supported tests and ocx_pipe_dispatch instantiates.
constexpr bool pipe_layout(int C, int P) {
    return ((P == 8 || P == 16 || P == 32) && (C == 4 || C == 8 || C == 16 || C == 32)) ||
           (P == 64 && C == 16);  // one sequence per wave: d = 1024
}

// ocx_launch_alg's rule, for every kernel built on the loop (OCX_ALG_NO_PIPE=1: the plain
// forms, for A/B measurements)
inline bool ocx_alg_use_pipe(const ocx_layout* L) {
    static const bool no_pipe = [] {
        const char* e = std::getenv("OCX_ALG_NO_PIPE");
        return e && std::atoi(e) != 0;
    }();
    return !no_pipe && ocx_pipe_supported(L);
}

// Waves per block of the full-form launch: four (a block spreads one wave to each SIMD of its
// CU, the last blocks three, ocx_pipe_wave_id) unless OCX_BLOCK_WAVES forces another shape or
// the launch has fewer than four groups.  That is the block's shape, not the residency: the
// 8 x 8 full form compiles to 212 VGPRs, two waves per SIMD, so a CU holds two such blocks and
// a launch of more than 2 x 4 x CUs groups would run in dispatcher rounds — such a batch takes
// the persistent launch instead (ocx_alg_pipe.hip, launch_pipe_cp).  The few-wave batches
// measured one-wave blocks (which the plain kernels keep below eight waves per CU) slower:
// profiles/r04_pipe_bw_ab.jsonl, r04_wave_clock*.jsonl.
inline int pipe_block_waves(int64_t G) {
    if (std::getenv("OCX_BLOCK_WAVES")) return ocx_block_waves(G);
    return G >= 4 ? 4 : 1;
}

// z_{t-1} .. z_{t+1} must be in the ring, and the late loads (ocx_ring_loop) keep NB-2
// steps in flight: one slot more than the plain kernel's ring
template <int C>
constexpr int pipe_nb(int P) {
    return nb_for(C, P) + 1 < 4 ? 4 : nb_for(C, P) + 1;
}

// The rescale test (RT) per kernel: measured (profiles/r04_pipe_ab3.jsonl) 3 328 x 1e5 at
// 16 x 4: 32.5 -> 28.7 ms; the pipeline's lean 8 x 8 form: 66.7 -> 64.3 ms per batch; but the
// 8 x 8 full form (the T = 1e5 batch): 40.8 -> 43.6 ms, which keeps the sqrt.
template <int C, int P, int MINW>
constexpr bool pipe_rt() {
    return !(C == 8 && P == 8 && MINW == 1);
}

// f(integral_constant C, integral_constant P) for L's layout, one instance per pipe_layout
template <int C, int P, class F>
bool pipe_dispatch_cp(const ocx_layout* L, F& f, hipError_t& e) {
    if constexpr (pipe_layout(C, P)) {
        if (L->C == C && L->P == P) {
            e = f(std::integral_constant<int, C>{}, std::integral_constant<int, P>{});
            return true;
        }
    }
    return false;
}
template <int C, class F>
bool pipe_dispatch_c(const ocx_layout* L, F& f, hipError_t& e) {
    return pipe_dispatch_cp<C, 8>(L, f, e) || pipe_dispatch_cp<C, 16>(L, f, e) ||
           pipe_dispatch_cp<C, 32>(L, f, e) || pipe_dispatch_cp<C, 64>(L, f, e);
}
template <class F>
hipError_t ocx_pipe_dispatch(const ocx_layout* L, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)(pipe_dispatch_c<4>(L, f, e) || pipe_dispatch_c<8>(L, f, e) ||
           pipe_dispatch_c<16>(L, f, e) || pipe_dispatch_c<32>(L, f, e));
    return e;
}
