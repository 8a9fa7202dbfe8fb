// BST's transformer block (algorithm/BST/transformer_layer.py:6-81), two kernels each way; include/recalgo_bst.h states the
// contract, DESIGN.md §5 "BST block" the layout and its LDS budget.
//
//   attn:  Xp = x + pos;  Q_h = Xp wq_h, K_h = Xp wk_h, V_h = x wv_h;  P_h = softmax(Q_h K_h^T / sqrt(d) + query-row mask);
//          n1 = LayerNorm(concat_h(P_h V_h) wo + Xp)
//   ffn:   out = LayerNorm(leakyrelu(n1 W + b) + n1);  pool = sum_t out (or the mean)
//
// Shape of all four kernels: a 512-thread workgroup works on ONE example at a time with the example's whole working set
// in LDS (T <= 64 rows of d <= 16 floats, one head's [T, T] probabilities), over a persistent grid: workgroup r takes the
// examples r, r + grid, ...  The parameters are staged in LDS once per workgroup.  Row-major [T, d] tiles have the row
// stride d + 1 and the probabilities T | 1: lanes that walk rows hit distinct banks.  Matrix products are plain FMA chains of
// at most 64 terms over fp32 tiles, ACCUMULATED IN DOUBLE and rounded once when the tile is stored: the backward's
// dS = P (dP - <P, dP>) cancels (all of it on a near-uniform row), so every fp32 rounding of Q, K, V, dA or dP ahead of it
// is amplified — with fp32 chains the T = 2 cases left 2.4 x as many elements outside the strict 1e-5 bound as the fp32
// reference arithmetic does.  The softmax of a row (one wave per row, one lane per key) and the LayerNorm moments are
// evaluated in double as well.  The backward kernels recompute the forward from its inputs (the attention one twice per head:
// once for concat_h(P_h V_h), which LayerNorm's backward needs first, once for the head's own gradients) and add every
// parameter gradient into an LDS accumulator whose entry i is only ever touched by thread i % 512: the workgroup's
// partial row, written once; recalgo_slabs::launch_colsums adds the rows in the fixed order of slab_sum.h.  No float
// atomics.
// The kernels are instantiated per d (4, 8, 12, 16): every loop over d unrolls, so its LDS reads are issued together.
#include "common.h"
#include "slab_sum.h"

#include "../../include/recalgo_bst.h"

namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;    // (1024 would cap a thread at 128 VGPRs: the attention backward spills there)
constexpr int kMaxT = RECALGO_BST_MAX_T, kMaxD = RECALGO_BST_MAX_D, kMaxH = RECALGO_BST_MAX_HEADS;
constexpr int kFwdGrid = 1024, kBwdGrid = 512;      // persistent grids
constexpr float kMaskAdd = -4294967296.0f;          // float32(-2^32 + 1)
constexpr double kLnEps = 1e-12;
constexpr int kRed = 2 * kWaves;                    // floats at the start of LDS: kWaves doubles of block_sum (8-byte aligned)

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the workgroup, the waves' sums added in wave order; every thread gets the result.  (Two barriers.)
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += red[w];
    __syncthreads();
    return s;
}

// acc + a * b in double
__device__ __forceinline__ double mad(float a, float b, double acc) { return fma((double)a, (double)b, acc); }

__device__ __forceinline__ void stage(float* dst, const float* __restrict__ src, int n) {
    for (int i = threadIdx.x; i < n; i += kThreads) dst[i] = src[i];
}

// ---- LDS layouts (floats) -----------------------------------------------------------------------------------------------
struct AttnLds {
    int ldd, lds, lda;                                              // row strides of [T, d], [T, T], [T, H d] tiles
    int wq, wk, wv, wo, pos, gam, bet, X, XP, Q, K, V, S, A, Y;     // both directions
    int DA, DY, DQ, DK, DV, DXP, DXV, ACC;                          // backward
    int a_pos, a_wq, a_wk, a_wv, a_wo, a_gam, a_bet, n_acc;         // offsets inside ACC = inside a partial row
    int total;
};

inline AttnLds attn_lds(int T, int d, int H, bool bwd) {
    AttnLds L;
    L.ldd = d + 1, L.lds = T | 1, L.lda = (H * d) | 1;
    int at = kRed;
    auto take = [&at](int n) { const int o = at; at += (n + 3) & ~3; return o; };
    L.wq = take(H * d * d), L.wk = take(H * d * d), L.wv = take(H * d * d), L.wo = take(H * d * d);
    L.pos = take(T * d), L.gam = take(d), L.bet = take(d);
    L.X = take(T * L.ldd), L.XP = take(T * L.ldd);
    L.Q = take(T * L.ldd), L.K = take(T * L.ldd), L.V = take(T * L.ldd);
    L.S = take(T * L.lds), L.A = take(T * L.lda), L.Y = take(T * L.ldd);
    L.a_pos = 0, L.a_wq = T * d, L.a_wk = L.a_wq + H * d * d, L.a_wv = L.a_wk + H * d * d, L.a_wo = L.a_wv + H * d * d;
    L.a_gam = L.a_wo + H * d * d, L.a_bet = L.a_gam + d, L.n_acc = L.a_bet + d;
    L.DA = L.DY = L.DQ = L.DK = L.DV = L.DXP = L.DXV = L.ACC = 0;
    if (bwd) {
        L.DA = take(T * L.lda), L.DY = take(T * L.ldd);
        L.DQ = take(T * L.ldd), L.DK = take(T * L.ldd), L.DV = take(T * L.ldd);
        L.DXP = take(T * L.ldd), L.DXV = take(T * L.ldd);
        L.ACC = take(L.n_acc);
    }
    L.total = at;
    return L;
}

struct FfnLds {
    int ldd;
    int w, b, gam, bet, N1, Hh, Y;
    int G, DH, ACC;
    int a_w, a_b, a_gam, a_bet, n_acc;
    int total;
};

inline FfnLds ffn_lds(int T, int d, bool bwd) {
    FfnLds L;
    L.ldd = d + 1;
    int at = kRed;
    auto take = [&at](int n) { const int o = at; at += (n + 3) & ~3; return o; };
    L.w = take(d * d), L.b = take(d), L.gam = take(d), L.bet = take(d);
    L.N1 = take(T * L.ldd), L.Hh = take(T * L.ldd), L.Y = take(T * L.ldd);
    L.a_w = 0, L.a_b = d * d, L.a_gam = L.a_b + d, L.a_bet = L.a_gam + d, L.n_acc = L.a_bet + d;
    L.G = L.DH = L.ACC = 0;
    if (bwd) L.G = take(T * L.ldd), L.DH = take(T * L.ldd), L.ACC = take(L.n_acc);
    L.total = at;
    return L;
}

// ---- the attention forward's pieces (shared with the backward's recomputation) ---------------------------------------------
struct AttnArgs {
    const float *x, *pos, *wq, *wk, *wv, *wo, *gamma, *beta;
    const int32_t* keys_length;
    int B, T, d, H;
    float scale;                    // sqrtf(d), rounded on the host
};

template <int D>
__device__ __forceinline__ void attn_stage_params(const AttnArgs& a, const AttnLds& L, float* sm) {
    const int n = a.H * D * D;
    stage(sm + L.wq, a.wq, n), stage(sm + L.wk, a.wk, n), stage(sm + L.wv, a.wv, n), stage(sm + L.wo, a.wo, n);
    stage(sm + L.pos, a.pos, a.T * D), stage(sm + L.gam, a.gamma, D);
    if (a.beta != nullptr) stage(sm + L.bet, a.beta, D);
}

__device__ __forceinline__ int clamped_length(const AttnArgs& a, int e) {
    const int kl = a.keys_length[e];
    return kl < 0 ? 0 : (kl > a.T ? a.T : kl);
}

// X = x[e], XP = x[e] + pos
template <int D>
__device__ __forceinline__ void attn_load(const AttnArgs& a, const AttnLds& L, float* sm, int e) {
    const int T = a.T, d = D;
    const float* xe = a.x + (size_t)e * T * d;
    for (int i = threadIdx.x; i < T * d; i += kThreads) {
        const int t = i / d, j = i - t * d;
        const float v = xe[i];
        sm[L.X + t * L.ldd + j] = v;
        sm[L.XP + t * L.ldd + j] = v + sm[L.pos + i];
    }
}

// Q, K, V of head h
template <int D>
__device__ __forceinline__ void attn_project(const AttnArgs& a, const AttnLds& L, float* sm, int h) {
    const int T = a.T, d = D, n = T * d;
    for (int i = threadIdx.x; i < 3 * n; i += kThreads) {
        const int m = i / n, r = i - m * n, t = r / d, j = r - t * d;
        const float* src = sm + (m == 2 ? L.X : L.XP) + t * L.ldd;
        const float* w = sm + (m == 0 ? L.wq : (m == 1 ? L.wk : L.wv)) + h * d * d + j;
        double s = 0.0;
        for (int c = 0; c < d; ++c) s = mad(src[c], w[c * d], s);
        sm[(m == 0 ? L.Q : (m == 1 ? L.K : L.V)) + t * L.ldd + j] = (float)s;
    }
}

// S = softmax over the keys of Q K^T / sqrt(d) (+ the mask constant on the query rows >= kl): a wave per row, a lane per key
template <int D>
__device__ __forceinline__ void attn_softmax(const AttnArgs& a, const AttnLds& L, float* sm, int kl) {
    const int T = a.T, d = D, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < T; i += kWaves) {
        float s = -INFINITY;
        if (lane < T) {
            const float *q = sm + L.Q + i * L.ldd, *k = sm + L.K + lane * L.ldd;
            double dot = 0.0;
            for (int c = 0; c < d; ++c) dot = mad(q[c], k[c], dot);
            s = (float)dot / a.scale;
            if (i >= kl) s = s + kMaskAdd;          // the literal fp32 add: every |s| < 128 is absorbed
        }
        const float m = wave_max(s);
        const double ex = lane < T ? exp((double)(s - m)) : 0.0;
        const double sum = wave_sum_d(ex);
        if (lane < T) sm[L.S + i * L.lds + lane] = (float)(ex / sum);
    }
}

// A[:, h d : (h + 1) d] = S V
template <int D>
__device__ __forceinline__ void attn_mix(const AttnArgs& a, const AttnLds& L, float* sm, int h) {
    const int T = a.T, d = D;
    for (int i = threadIdx.x; i < T * d; i += kThreads) {
        const int t = i / d, j = i - t * d;
        const float *p = sm + L.S + t * L.lds, *v = sm + L.V + j;
        double s = 0.0;
        for (int k = 0; k < T; ++k) s = mad(p[k], v[k * L.ldd], s);
        sm[L.A + t * L.lda + h * d + j] = (float)s;
    }
}

// Y = A wo + XP
template <int D>
__device__ __forceinline__ void attn_output(const AttnArgs& a, const AttnLds& L, float* sm) {
    const int T = a.T, d = D, HD = a.H * D;
    for (int i = threadIdx.x; i < T * d; i += kThreads) {
        const int t = i / d, j = i - t * d;
        const float *ar = sm + L.A + t * L.lda, *w = sm + L.wo + j;
        double s = 0.0;
        for (int c = 0; c < HD; ++c) s = mad(ar[c], w[c * d], s);
        sm[L.Y + t * L.ldd + j] = (float)(s + (double)sm[L.XP + t * L.ldd + j]);
    }
}

// the whole forward of example e up to Y (the caller has loaded X / XP and synchronized)
template <int D>
__device__ __forceinline__ void attn_forward_to_y(const AttnArgs& a, const AttnLds& L, float* sm, int kl) {
    for (int h = 0; h < a.H; ++h) {
        attn_project<D>(a, L, sm, h);
        __syncthreads();
        attn_softmax<D>(a, L, sm, kl);
        __syncthreads();
        attn_mix<D>(a, L, sm, h);
        __syncthreads();            // (the next head overwrites Q, K, V, S)
    }
    attn_output<D>(a, L, sm);
    __syncthreads();
}

// mean and 1 / sqrt(var + eps) of the [T, d] tile at `y` (row stride ldd), in double; two passes
__device__ __forceinline__ void moments(const float* y, int T, int d, int ldd, double* red, double* mean, double* rstd) {
    const int n = T * d;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) s += (double)y[(i / d) * ldd + i % d];
    const double mu = block_sum(s, red) / n;
    s = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const double c = (double)y[(i / d) * ldd + i % d] - mu;
        s = fma(c, c, s);
    }
    const double var = block_sum(s, red) / n;
    *mean = mu, *rstd = 1.0 / sqrt(var + kLnEps);
}

template <int D>
__global__ __launch_bounds__(kThreads) void bst_attn_fwd_kernel(AttnArgs a, AttnLds L, float* __restrict__ n1, float* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    double* red = reinterpret_cast<double*>(sm);
    const int T = a.T, d = D;
    attn_stage_params<D>(a, L, sm);
    __syncthreads();
    for (int e = blockIdx.x; e < a.B; e += gridDim.x) {
        attn_load<D>(a, L, sm, e);
        __syncthreads();
        attn_forward_to_y<D>(a, L, sm, clamped_length(a, e));
        double mean, rstd;
        moments(sm + L.Y, T, d, L.ldd, red, &mean, &rstd);
        float* out = n1 + (size_t)e * T * d;
        for (int i = threadIdx.x; i < T * d; i += kThreads) {
            const int t = i / d, j = i - t * d;
            const float xh = (float)(((double)sm[L.Y + t * L.ldd + j] - mean) * rstd);
            out[i] = fmaf(xh, sm[L.gam + j], sm[L.bet + j]);
        }
        if (stats != nullptr && threadIdx.x == 0) stats[2 * e] = (float)mean, stats[2 * e + 1] = (float)rstd;
        __syncthreads();            // (the next example overwrites X, XP, Y)
    }
}

// LayerNorm's backward on the tile: `xh` holds y (becomes xhat in place), `g` the upstream gradient (becomes dy in place);
// dgamma / dbeta of the example are added to acc_g / acc_b.  On return every thread may read xh and g.
__device__ __forceinline__ void layer_norm_bwd(float* xh, float* g, const float* gam, float* acc_g, float* acc_b, int T, int d,
                                               int ldd, double* red) {
    double mean, rstd;
    moments(xh, T, d, ldd, red, &mean, &rstd);
    const int n = T * d;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int at = (i / d) * ldd + i % d;
        const float h = (float)(((double)xh[at] - mean) * rstd);
        xh[at] = h;
        const double gh = (double)g[at] * (double)gam[i % d];
        s1 += gh, s2 = fma(gh, (double)h, s2);
    }
    const double m1 = block_sum(s1, red) / n, m2 = block_sum(s2, red) / n;        // (barriers: xh is complete)
    if ((int)threadIdx.x < d) {
        const int j = threadIdx.x;
        double ga = 0.0, be = 0.0;
        for (int t = 0; t < T; ++t) ga = mad(g[t * ldd + j], xh[t * ldd + j], ga), be += (double)g[t * ldd + j];
        acc_g[j] += (float)ga, acc_b[j] += (float)be;
    }
    __syncthreads();                // (g is overwritten next)
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int at = (i / d) * ldd + i % d;
        const double gh = (double)g[at] * (double)gam[i % d];
        g[at] = (float)(rstd * (gh - m1 - (double)xh[at] * m2));
    }
    __syncthreads();
}

template <int D>
__global__ __launch_bounds__(kThreads) void bst_attn_bwd_kernel(AttnArgs a, AttnLds L, const float* __restrict__ g_n1, float* __restrict__ dx,
                                                                float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    double* red = reinterpret_cast<double*>(sm);
    const int T = a.T, d = D, H = a.H, HD = H * d, n = T * d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* acc = sm + L.ACC;
    attn_stage_params<D>(a, L, sm);
    for (int i = threadIdx.x; i < L.n_acc; i += kThreads) acc[i] = 0.f;
    __syncthreads();
    for (int e = blockIdx.x; e < a.B; e += gridDim.x) {
        const int kl = clamped_length(a, e);
        attn_load<D>(a, L, sm, e);
        const float* ge = g_n1 + (size_t)e * n;
        for (int i = threadIdx.x; i < n; i += kThreads) sm[L.DY + (i / d) * L.ldd + i % d] = ge[i];
        __syncthreads();
        attn_forward_to_y<D>(a, L, sm, kl);
        layer_norm_bwd(sm + L.Y, sm + L.DY, sm + L.gam, acc + L.a_gam, acc + L.a_bet, T, d, L.ldd, red);
        // dA = dY wo^T;  dwo += A^T dY;  the residual: dXP = dY, dXV = 0
        for (int i = threadIdx.x; i < T * HD; i += kThreads) {
            const int t = i / HD, c = i - t * HD;
            const float *dy = sm + L.DY + t * L.ldd, *w = sm + L.wo + c * d;
            double s = 0.0;
            for (int j = 0; j < d; ++j) s = mad(dy[j], w[j], s);
            sm[L.DA + t * L.lda + c] = (float)s;
        }
        for (int i = threadIdx.x; i < HD * d; i += kThreads) {
            const int c = i / d, j = i - c * d;
            double s = 0.0;
            for (int t = 0; t < T; ++t) s = mad(sm[L.A + t * L.lda + c], sm[L.DY + t * L.ldd + j], s);
            acc[L.a_wo + i] += (float)s;
        }
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int at = (i / d) * L.ldd + i % d;
            sm[L.DXP + at] = sm[L.DY + at], sm[L.DXV + at] = 0.f;
        }
        __syncthreads();
        for (int h = 0; h < H; ++h) {
            attn_project<D>(a, L, sm, h);
            __syncthreads();
            attn_softmax<D>(a, L, sm, kl);
            __syncthreads();
            // dV = P^T dO   (dO = dA[:, h d : (h + 1) d])
            for (int i = threadIdx.x; i < n; i += kThreads) {
                const int k = i / d, j = i - k * d;
                double s = 0.0;
                for (int q = 0; q < T; ++q) s = mad(sm[L.S + q * L.lds + k], sm[L.DA + q * L.lda + h * d + j], s);
                sm[L.DV + k * L.ldd + j] = (float)s;
            }
            __syncthreads();
            // dS = P (dP - <P, dP>) / sqrt(d), in place of P: a wave per row, a lane per key
            for (int q = wave; q < T; q += kWaves) {
                float p = 0.f;
                double dp = 0.0;
                if (lane < T) {
                    const float *dO = sm + L.DA + q * L.lda + h * d, *v = sm + L.V + lane * L.ldd;
                    for (int j = 0; j < d; ++j) dp = mad(dO[j], v[j], dp);
                    p = sm[L.S + q * L.lds + lane];
                }
                const double dot = wave_sum_d((double)p * dp);
                if (lane < T) sm[L.S + q * L.lds + lane] = (float)((double)p * (dp - dot) / (double)a.scale);
            }
            __syncthreads();
            // dQ = dS K, dK = dS^T Q
            for (int i = threadIdx.x; i < 2 * n; i += kThreads) {
                const int m = i / n, r = i - m * n, t = r / d, j = r - t * d;
                double s = 0.0;
                if (m == 0) {
                    for (int k = 0; k < T; ++k) s = mad(sm[L.S + t * L.lds + k], sm[L.K + k * L.ldd + j], s);
                    sm[L.DQ + t * L.ldd + j] = (float)s;
                } else {
                    for (int q = 0; q < T; ++q) s = mad(sm[L.S + q * L.lds + t], sm[L.Q + q * L.ldd + j], s);
                    sm[L.DK + t * L.ldd + j] = (float)s;
                }
            }
            __syncthreads();
            // dwq_h += XP^T dQ, dwk_h += XP^T dK, dwv_h += X^T dV
            for (int i = threadIdx.x; i < 3 * d * d; i += kThreads) {
                const int m = i / (d * d), r = i - m * d * d, c = r / d, j = r - c * d;
                const float* src = sm + (m == 2 ? L.X : L.XP) + c;
                const float* dm = sm + (m == 0 ? L.DQ : (m == 1 ? L.DK : L.DV)) + j;
                double s = 0.0;
                for (int t = 0; t < T; ++t) s = mad(src[t * L.ldd], dm[t * L.ldd], s);
                acc[(m == 0 ? L.a_wq : (m == 1 ? L.a_wk : L.a_wv)) + h * d * d + r] += (float)s;
            }
            // dXP += dQ wq_h^T + dK wk_h^T, dXV += dV wv_h^T
            for (int i = threadIdx.x; i < n; i += kThreads) {
                const int t = i / d, c = i - t * d;
                const float *dq = sm + L.DQ + t * L.ldd, *dk = sm + L.DK + t * L.ldd, *dv = sm + L.DV + t * L.ldd;
                const float *wq = sm + L.wq + h * d * d + c * d, *wk = sm + L.wk + h * d * d + c * d;
                const float* wv = sm + L.wv + h * d * d + c * d;
                double sp = (double)sm[L.DXP + t * L.ldd + c], sv = (double)sm[L.DXV + t * L.ldd + c];
                for (int j = 0; j < d; ++j) sp = mad(dq[j], wq[j], sp);
                for (int j = 0; j < d; ++j) sp = mad(dk[j], wk[j], sp);
                for (int j = 0; j < d; ++j) sv = mad(dv[j], wv[j], sv);
                sm[L.DXP + t * L.ldd + c] = (float)sp, sm[L.DXV + t * L.ldd + c] = (float)sv;
            }
            __syncthreads();
        }
        float* dxe = dx + (size_t)e * n;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int at = (i / d) * L.ldd + i % d;
            const float gp = sm[L.DXP + at];
            dxe[i] = (float)((double)gp + (double)sm[L.DXV + at]);
            acc[L.a_pos + i] += gp;
        }
        __syncthreads();            // (the next example overwrites every tile)
    }
    float* prow = partials + (size_t)blockIdx.x * L.n_acc;
    for (int i = threadIdx.x; i < L.n_acc; i += kThreads) prow[i] = acc[i];
}

// ---- FFN ---------------------------------------------------------------------------------------------------------------------
struct FfnArgs {
    const float *n1, *w, *b, *gamma, *beta;
    int B, T, d, mean_pool;
};

template <int D>
__device__ __forceinline__ void ffn_stage_params(const FfnArgs& a, const FfnLds& L, float* sm) {
    stage(sm + L.w, a.w, D * D), stage(sm + L.b, a.b, D), stage(sm + L.gam, a.gamma, D);
    if (a.beta != nullptr) stage(sm + L.bet, a.beta, D);
}

// N1 = n1[e];  Hh = N1 W + b;  Y = leakyrelu(Hh) + N1
template <int D>
__device__ __forceinline__ void ffn_forward_to_y(const FfnArgs& a, const FfnLds& L, float* sm, int e) {
    const int T = a.T, d = D, n = T * d;
    const float* src = a.n1 + (size_t)e * n;
    for (int i = threadIdx.x; i < n; i += kThreads) sm[L.N1 + (i / d) * L.ldd + i % d] = src[i];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int t = i / d, j = i - t * d;
        const float *r = sm + L.N1 + t * L.ldd, *w = sm + L.w + j;
        double s = 0.0;
        for (int c = 0; c < d; ++c) s = mad(r[c], w[c * d], s);
        s += (double)sm[L.b + j];
        sm[L.Hh + t * L.ldd + j] = (float)s;            // (the backward needs its sign)
        sm[L.Y + t * L.ldd + j] = (float)((0.505 * s + 0.495 * fabs(s)) + (double)r[j]);
    }
    __syncthreads();
}

template <int D>
__global__ __launch_bounds__(kThreads) void bst_ffn_fwd_kernel(FfnArgs a, FfnLds L, float* __restrict__ out, float* __restrict__ pool,
                                                               float* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    double* red = reinterpret_cast<double*>(sm);
    const int T = a.T, d = D, n = T * d;
    ffn_stage_params<D>(a, L, sm);
    __syncthreads();
    for (int e = blockIdx.x; e < a.B; e += gridDim.x) {
        ffn_forward_to_y<D>(a, L, sm, e);
        double mean, rstd;
        moments(sm + L.Y, T, d, L.ldd, red, &mean, &rstd);
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int t = i / d, j = i - t * d;
            const float xh = (float)(((double)sm[L.Y + t * L.ldd + j] - mean) * rstd);
            const float o = fmaf(xh, sm[L.gam + j], sm[L.bet + j]);
            if (out != nullptr) out[(size_t)e * n + i] = o;
            sm[L.Hh + t * L.ldd + j] = o;          // (each thread overwrites only the elements it has just read as Y's)
        }
        if (stats != nullptr && threadIdx.x == 0) stats[2 * e] = (float)mean, stats[2 * e + 1] = (float)rstd;
        __syncthreads();
        if (pool != nullptr && (int)threadIdx.x < d) {
            double s = 0.0;
            for (int t = 0; t < T; ++t) s += (double)sm[L.Hh + t * L.ldd + threadIdx.x];
            pool[(size_t)e * d + threadIdx.x] = (float)(a.mean_pool ? s / T : s);
        }
        __syncthreads();            // (the next example overwrites N1, Hh, Y)
    }
}

template <int D>
__global__ __launch_bounds__(kThreads) void bst_ffn_bwd_kernel(FfnArgs a, FfnLds L, const float* __restrict__ g_out,
                                                               const float* __restrict__ g_pool, float* __restrict__ dn1,
                                                               float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    double* red = reinterpret_cast<double*>(sm);
    const int T = a.T, d = D, n = T * d;
    float* acc = sm + L.ACC;
    ffn_stage_params<D>(a, L, sm);
    for (int i = threadIdx.x; i < L.n_acc; i += kThreads) acc[i] = 0.f;
    __syncthreads();
    for (int e = blockIdx.x; e < a.B; e += gridDim.x) {
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int j = i % d;
            float g = g_out != nullptr ? g_out[(size_t)e * n + i] : 0.f;
            if (g_pool != nullptr) {
                const float gp = g_pool[(size_t)e * d + j];
                g += a.mean_pool ? gp / (float)T : gp;
            }
            sm[L.G + (i / d) * L.ldd + j] = g;
        }
        ffn_forward_to_y<D>(a, L, sm, e);              // (its barriers publish G as well)
        layer_norm_bwd(sm + L.Y, sm + L.G, sm + L.gam, acc + L.a_gam, acc + L.a_bet, T, d, L.ldd, red);
        // dH = dY leakyrelu'(H)
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int at = (i / d) * L.ldd + i % d;
            const float h = sm[L.Hh + at];
            const float sg = h > 0.f ? 1.f : (h < 0.f ? -1.f : 0.f);
            sm[L.DH + at] = sm[L.G + at] * (0.505f + 0.495f * sg);
        }
        __syncthreads();
        // dn1 = dY + dH W^T;  dW += N1^T dH;  db += sum_t dH
        float* dst = dn1 + (size_t)e * n;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int t = i / d, c = i - t * d;
            const float *dh = sm + L.DH + t * L.ldd, *w = sm + L.w + c * d;
            double s = (double)sm[L.G + t * L.ldd + c];
            for (int j = 0; j < d; ++j) s = mad(dh[j], w[j], s);
            dst[i] = (float)s;
        }
        for (int i = threadIdx.x; i < d * d + d; i += kThreads) {
            double s = 0.0;
            if (i < d * d) {
                const int c = i / d, j = i - c * d;
                for (int t = 0; t < T; ++t) s = mad(sm[L.N1 + t * L.ldd + c], sm[L.DH + t * L.ldd + j], s);
            } else {
                for (int t = 0; t < T; ++t) s += (double)sm[L.DH + t * L.ldd + (i - d * d)];
            }
            acc[i] += (float)s;            // (a_w = 0, a_b = d d: one run)
        }
        __syncthreads();            // (the next example overwrites every tile)
    }
    float* prow = partials + (size_t)blockIdx.x * L.n_acc;
    for (int i = threadIdx.x; i < L.n_acc; i += kThreads) prow[i] = acc[i];
}

bool shape_ok(int T, int d, int H) {
    return T >= 1 && T <= kMaxT && d >= 4 && d <= kMaxD && (d & 3) == 0 && H >= 1 && H <= kMaxH &&
           sizeof(float) * (size_t)attn_lds(T, d, H, true).total <= kLdsMax;
}

int rows_for(int B, int cap) { return B < 1 ? 1 : (B > cap ? cap : B); }

// launch_lds raises the dynamic-LDS allowance of the instantiation it launches (d is one of 4, 8, 12, 16: shape_ok)
#define BST_LAUNCH(KERNEL, d, grid, lds, st, ...)                                                          \
    RECALGO_CHECK((d) == 4    ? launch_lds<KERNEL<4>>(grid, dim3(kThreads), lds, st, __VA_ARGS__)          \
                  : (d) == 8  ? launch_lds<KERNEL<8>>(grid, dim3(kThreads), lds, st, __VA_ARGS__)          \
                  : (d) == 12 ? launch_lds<KERNEL<12>>(grid, dim3(kThreads), lds, st, __VA_ARGS__)         \
                              : launch_lds<KERNEL<16>>(grid, dim3(kThreads), lds, st, __VA_ARGS__))

}  // namespace

RECALGO_EXPORT int recalgo_bst_abi_version(void) { return RECALGO_BST_ABI_VERSION; }

RECALGO_EXPORT int recalgo_bst_supported(int T, int d, int H) { return shape_ok(T, d, H) ? 1 : 0; }

RECALGO_EXPORT int recalgo_bst_attn_bwd_partial_rows(int B) { return rows_for(B, kBwdGrid); }

RECALGO_EXPORT int64_t recalgo_bst_attn_bwd_workspace_bytes(int B, int T, int d, int H) {
    if (!shape_ok(T, d, H)) return 0;
    return (int64_t)sizeof(float) * rows_for(B, kBwdGrid) * attn_lds(T, d, H, true).n_acc;
}

RECALGO_EXPORT int recalgo_bst_ffn_bwd_partial_rows(int B) { return rows_for(B, kBwdGrid); }

RECALGO_EXPORT int64_t recalgo_bst_ffn_bwd_workspace_bytes(int B, int d) {
    if (!shape_ok(1, d, 1)) return 0;
    return (int64_t)sizeof(float) * rows_for(B, kBwdGrid) * ffn_lds(1, d, true).n_acc;
}

RECALGO_EXPORT int recalgo_bst_attn_fwd(const float* x, const float* pos, const int32_t* keys_length, const float* w_q,
                                        const float* w_k, const float* w_v, const float* w_o, const float* gamma,
                                        const float* beta, int B, int T, int d, int H, float* n1, float* stats,
                                        recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, d, H));
    RECALGO_REQUIRE(x && pos && keys_length && w_q && w_k && w_v && w_o && gamma && beta && n1);
    RECALGO_REQUIRE(aligned_to<4>(x, pos, w_q, w_k, w_v, w_o, gamma, beta, n1, stats) && aligned_to<4>(keys_length));
    const AttnArgs a = {x, pos, w_q, w_k, w_v, w_o, gamma, beta, keys_length, B, T, d, H, sqrtf((float)d)};
    const AttnLds L = attn_lds(T, d, H, false);      // (the layout travels as a kernel argument)
    BST_LAUNCH(bst_attn_fwd_kernel, d, dim3(rows_for(B, kFwdGrid)), sizeof(float) * (size_t)L.total, as_stream(stream), a, L, n1, stats);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_bst_attn_bwd(const float* x, const float* pos, const int32_t* keys_length, const float* w_q,
                                        const float* w_k, const float* w_v, const float* w_o, const float* gamma,
                                        const float* g_n1, int B, int T, int d, int H, float* dx, float* dpos, float* dw_q,
                                        float* dw_k, float* dw_v, float* dw_o, float* dgamma, float* dbeta, float* workspace,
                                        recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, d, H));
    RECALGO_REQUIRE(x && pos && keys_length && w_q && w_k && w_v && w_o && gamma && g_n1);
    RECALGO_REQUIRE(dx && dpos && dw_q && dw_k && dw_v && dw_o && dgamma && dbeta && workspace);
    RECALGO_REQUIRE(aligned_to<4>(x, pos, w_q, w_k, w_v, w_o, gamma, g_n1) && aligned_to<4>(keys_length));
    RECALGO_REQUIRE(aligned_to<4>(dx, dpos, dw_q, dw_k, dw_v, dw_o, dgamma, dbeta, workspace));
    const AttnArgs a = {x, pos, w_q, w_k, w_v, w_o, gamma, nullptr, keys_length, B, T, d, H, sqrtf((float)d)};
    const AttnLds L = attn_lds(T, d, H, true);
    const int rows = rows_for(B, kBwdGrid);
    hipStream_t st = as_stream(stream);
    BST_LAUNCH(bst_attn_bwd_kernel, d, dim3(rows), sizeof(float) * (size_t)L.total, st, a, L, g_n1, dx, workspace);
    float* const outs[7] = {dpos, dw_q, dw_k, dw_v, dw_o, dgamma, dbeta};
    const int starts[8] = {L.a_pos, L.a_wq, L.a_wk, L.a_wv, L.a_wo, L.a_gam, L.a_bet, L.n_acc};
    return recalgo_slabs::launch_colsums(workspace, rows, 7, outs, starts, st);
}

RECALGO_EXPORT int recalgo_bst_ffn_fwd(const float* n1, const float* ffn_w, const float* ffn_b, const float* gamma,
                                       const float* beta, int B, int T, int d, int mean_pool, float* out, float* pool,
                                       float* stats, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, d, 1));
    RECALGO_REQUIRE(n1 && ffn_w && ffn_b && gamma && beta && (out || pool));
    RECALGO_REQUIRE(aligned_to<4>(n1, ffn_w, ffn_b, gamma, beta, out, pool, stats));
    const FfnArgs a = {n1, ffn_w, ffn_b, gamma, beta, B, T, d, mean_pool != 0};
    const FfnLds L = ffn_lds(T, d, false);
    BST_LAUNCH(bst_ffn_fwd_kernel, d, dim3(rows_for(B, kFwdGrid)), sizeof(float) * (size_t)L.total, as_stream(stream), a, L, out, pool, stats);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_bst_ffn_bwd(const float* n1, const float* ffn_w, const float* ffn_b, const float* gamma,
                                       const float* g_out, const float* g_pool, int B, int T, int d, int mean_pool, float* dn1,
                                       float* dw, float* db, float* dgamma, float* dbeta, float* workspace,
                                       recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(T, d, 1));
    RECALGO_REQUIRE(n1 && ffn_w && ffn_b && gamma && (g_out || g_pool) && dn1 && dw && db && dgamma && dbeta && workspace);
    RECALGO_REQUIRE(aligned_to<4>(n1, ffn_w, ffn_b, gamma, g_out, g_pool, dn1, dw, db, dgamma, dbeta, workspace));
    const FfnArgs a = {n1, ffn_w, ffn_b, gamma, nullptr, B, T, d, mean_pool != 0};
    const FfnLds L = ffn_lds(T, d, true);
    const int rows = rows_for(B, kBwdGrid);
    hipStream_t st = as_stream(stream);
    BST_LAUNCH(bst_ffn_bwd_kernel, d, dim3(rows), sizeof(float) * (size_t)L.total, st, a, L, g_out, g_pool, dn1, workspace);
    float* const outs[4] = {dw, db, dgamma, dbeta};
    const int starts[5] = {L.a_w, L.a_b, L.a_gam, L.a_bet, L.n_acc};
    return recalgo_slabs::launch_colsums(workspace, rows, 4, outs, starts, st);
}
