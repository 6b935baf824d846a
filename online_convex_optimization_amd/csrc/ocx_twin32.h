// ocx_twin32.h — the float32 twin's device arithmetic, shared by ocx_twin32.hip and
// ocx_twin32_cols.hip: the NumPy / OpenBLAS operation orders the twin's calls compute
// (ocx_twin32.hip's header comment) and the one-wave-per-sequence prefix sum.
// One copy: both files carry the same bits by construction.  Compiled with the flags of
// _build.py (no contraction) in either file.
#ifndef OCX_TWIN32_H_
#define OCX_TWIN32_H_

#include <cstdint>

#include "ocx_internal.h"

namespace {

constexpr int kPwBlock = 128;  // PW_BLOCKSIZE: the leaves of the pairwise recursion

// correctly rounded float sqrt and division, through double: 53 >= 2*24 + 2 bits, so the
// second rounding never changes the result (the float intrinsics here are not all rte)
__device__ __forceinline__ float t32_sqrt(float x) { return (float)sqrt((double)x); }
__device__ __forceinline__ float t32_div(float a, float b) { return (float)((double)a / (double)b); }

__device__ __forceinline__ float t32_tree8(const float (&r)[8]) {
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// sdot, n < 32: float products summed in double (padding coordinates add +0)
template <int C>
__device__ __forceinline__ float t32_sdot(const float (&a)[C], const float (&b)[C]) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < C; ++j) acc += (double)(a[j] * b[j]);
    return (float)acc;
}

// row i of an n-row sgemv z @ x
template <int C>
__device__ __forceinline__ float t32_gemv_row(const float (&z)[C], const float (&x)[C], int64_t i,
                                              int64_t n) {
    if (n == 1) return t32_sdot<C>(z, x);
    float a = 0.0f;
    if (i < (n & ~(int64_t)3)) {
#pragma unroll
        for (int j = 0; j < C; ++j) a = fmaf(z[j], x[j], a);
    } else {
#pragma unroll
        for (int j = 0; j < C; ++j) a = a + z[j] * x[j];
    }
    return a;
}

// _action_ftl (algorithms.py:13-15)
template <int C>
__device__ __forceinline__ void t32_ftl(const float (&th)[C], float (&x)[C]) {
    const float n = t32_sqrt(t32_sdot<C>(th, th));
    const float s = n == 0.0f ? 0.0f : -t32_div(1.0f, n);
#pragma unroll
    for (int j = 0; j < C; ++j) x[j] = n == 0.0f ? 0.0f : s * th[j];
}

// _action_ftrl (algorithms.py:17-21)
template <int C>
__device__ __forceinline__ void t32_ftrl(const float (&th)[C], int64_t t, double eta0,
                                         float (&x)[C]) {
    const float sc = (float)(-(eta0 / sqrt((double)(t > 1 ? t : 1))));
#pragma unroll
    for (int j = 0; j < C; ++j) x[j] = sc * th[j];
    const float n = t32_sqrt(t32_sdot<C>(x, x));
    if (n > 1.0f) {
        const float inv = t32_div(1.0f, n);
#pragma unroll
        for (int j = 0; j < C; ++j) x[j] = x[j] * inv;
    }
}

__device__ __forceinline__ double t32_grad(double diff) {
    return diff > 0.0 ? 0.5 : (diff < 0.0 ? -0.5 : 0.0);
}

// ---- one wavefront per sequence ---------------------------------------------------------
// simulate_SMART_like re-sums its whole prefix every step before the switch (:109-111):
// O(T^2) work per sequence, latency-bound in a lane of its own (T = 1000: 0.3 s for one
// sequence, against ~20 ms for NumPy).  Here the sequence's rows sit in LDS as float and
// the wave splits each prefix sum the way NumPy's pairwise recursion does: its leaves (of
// <= 128 losses, all starting at multiples of 8) and their eight accumulator chains are
// independent, so lane 8*i + k runs chain k of leaf i; lane 8*i then folds the chains
// (tree of 8) and the leaf's tail, and the leaf sums are combined in the recursion's post
// order.  The scalar part of the step (actions, theta updates) runs on every lane alike.
constexpr int kWaveLeaves = 128;  // leaves of an 8192-element buffer: at most 8192/64

struct T32Wave {
    const float* z;  // LDS rows [T][C]
    const float* y;  // LDS labels [T]
    float* red;      // [64]
    int* lstart;     // [kWaveLeaves]
    int* llen;
    float* lsum;
};

template <int C>
__device__ __forceinline__ float t32_wave_loss(const T32Wave& w, const float (&x)[C], int i, int n) {
    float zr[C];
#pragma unroll
    for (int j = 0; j < C; ++j) zr[j] = w.z[i * C + j];
    return 0.5f * fabsf(t32_gemv_row<C>(zr, x, i, n) - w.y[i]);
}

// np.sum(0.5 * np.abs(z[:n] @ x - y[:n])), n <= 8192 (one NumPy buffer), on the whole wave
template <int C>
__device__ float t32_wave_loss_sum(const T32Wave& w, const float (&x)[C], int n, int lane) {
    if (n == 0) return 0.0f;
    // the leaves, in order
    int nl = 0;
    {
        int stk[8];
        int sp = 0, m = n, pos = 0;
        for (;;) {
            while (m > kPwBlock) {
                int m2 = m / 2;
                m2 -= m2 % 8;
                stk[sp++] = m - m2;
                m = m2;
            }
            if (lane == 0) {
                w.lstart[nl] = pos;
                w.llen[nl] = m;
            }
            ++nl;
            pos += m;
            if (sp == 0) break;
            m = stk[--sp];
        }
    }
    __syncthreads();
    for (int base = 0; base < nl; base += 8) {
        const int leaf = base + (lane >> 3), k = lane & 7;
        int s = 0, m = 0;
        if (leaf < nl) {
            s = w.lstart[leaf];
            m = w.llen[leaf];
        }
        const int mfull = m - (m & 7);
        float r = 0.0f;
        if (m >= 8) {
            r = t32_wave_loss<C>(w, x, s + k, n);
            for (int i = s + k + 8; i < s + mfull; i += 8) r = r + t32_wave_loss<C>(w, x, i, n);
        }
        w.red[lane] = r;
        __syncthreads();
        if (k == 0 && leaf < nl) {
            float res;
            int i0;
            if (m >= 8) {
                float rr[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) rr[u] = w.red[lane + u];
                res = t32_tree8(rr);
                i0 = s + mfull;
            } else {
                res = -0.0f;
                i0 = s;
            }
            for (int i = i0; i < s + m; ++i) res = res + t32_wave_loss<C>(w, x, i, n);
            w.lsum[leaf] = res;
        }
        __syncthreads();
    }
    // the recursion's post order over the leaf sums
    int fr_len[8];
    float fr_val[8];
    bool fr_has[8];
    int sp = 0, m = n, li = 0;
    for (;;) {
        while (m > kPwBlock) {
            int m2 = m / 2;
            m2 -= m2 % 8;
            fr_len[sp] = m - m2;
            fr_has[sp] = false;
            ++sp;
            m = m2;
        }
        float v = w.lsum[li++];
        while (sp > 0 && fr_has[sp - 1]) {
            v = fr_val[sp - 1] + v;
            --sp;
        }
        if (sp == 0) {
            __syncthreads();  // leaf arrays are rewritten by the next call
            return v;
        }
        fr_val[sp - 1] = v;
        fr_has[sp - 1] = true;
        m = fr_len[sp - 1];
    }
}

constexpr int64_t kWaveLdsBytes = 60 * 1024;  // rows of one sequence staged in LDS (<= 64 KB with the static arrays)

}  // namespace

#endif  // OCX_TWIN32_H_
