// AutoInt's interacting layer (include/recalgo_autoint.h; Song et al., CIKM 2019, eqs. 5-8), one kernel each way.
//
// One wave per example, up to four waves per workgroup.  Every product is a set of v_mfma_f32_16x16x4_f32 tiles whose operands
// are read from LDS: lane l = (r, q) = (l & 15, l >> 4) supplies A[m = r][k = q] and B[k = q][n = r] of a k-step and receives
// C[m = 4 q + i][n = r] in register i.  F is built in tiles of 16, the last one masked.
//
// LDS.  Shared by the workgroup: the weights W[d][p C16 + c], p = 0..3 for Wq, Wk, Wv, Wres and c = h A + a the head-major
// column (C16 = H A rounded up to 16), so a projection is x times ONE [D, 3 H A] matrix.  Per wave: X [F16][D16 + 1],
// Q, K, V [F16][C16 + 1] and, in the backward, dZ [F16][C16 + 1], one head's dQ [F16][33] and three statistics of every query
// row.  The whole LDS is zeroed once; the rows f >= F and the columns past D, H A are never written with anything but zeros, so
// a masked row or column contributes exactly 0 to every sum that runs over it and no operand needs a mask of its own.
//
// The scores are formed TRANSPOSED: S^T = mfma(K rows, Q rows) leaves lane (r, q) with S[f = r][j = 4 q + i] of a key tile: a
// query row's softmax is an in-lane reduction and a butterfly over the four lane groups, a masked key gets -inf and so weight
// exactly 0, and the tile IS the A operand of P V (an MFMA's k-order is free: lane group q pairs P[f][4 q + i] with
// V[4 q + i][a]) — the scores never leave the registers.  The residual term x Wres starts the accumulator P V is added to.
//
// The backward recomputes Q, K, V, S^T and P the same way, dZ = g [y > 0] lies in LDS, dP^T = mfma(V rows, dZ rows) has the
// layout of P, dS follows in registers and is the A operand of dQ = dS K as it stands.  dK = dS^T Q and dV = P^T dZ need the
// other orientation, so a head is walked twice: by query tile for dQ and the row statistics (max, sum, rowsum(P dP)), then by
// key tile, where S and dP are formed as mfma(Q rows, K rows) and mfma(dZ rows, V rows) — lane (r, q) holds f = 4 q + i,
// j = r — and P, dS follow from the statistics: dK and dV of a key tile are four accumulators, nothing is transposed through
// LDS, and they take the place of the tile's K and V.  dQ replaces the head's Q at the end, and the example ends with two
// products: dx = [dQ|dK|dV|dZ] W^T and dW += X^T [dQ|dK|dV|dZ].  dW stays in registers over all examples of the wave (the
// kernel is instantiated per count of 16-row / 16-column tiles so that it holds exactly the accumulators the shape needs and
// every LDS stride is a constant, and from nine tile pairs on it walks its examples twice, for [dWq | dWk] and for
// [dWv | dWres]); at the end the waves of a workgroup add theirs in wave order into ONE partial row [dWq | dWk | dWv | dWres]
// in global memory, and recalgo_slabs::launch_colsums sums the rows.  Nothing depends on B or on which wave or workgroup
// serves an example.
#include "common.h"
#include "slab_sum.h"
#include "../../include/recalgo_autoint.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxWaves = 4;
constexpr int kMaxJT = RECALGO_AUTOINT_MAX_F / 16;
constexpr int kFwdGrid = 1024;
constexpr int kBwdGrid = RECALGO_AUTOINT_MAX_PARTIAL_ROWS;
constexpr int kLdq = RECALGO_AUTOINT_MAX_A + 1;       // row stride of a head's dQ
constexpr int kStat = RECALGO_AUTOINT_MAX_F;          // a row statistic of every query row

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// acc += sum over n k-steps of a[s * as] * b[s * bs]: the caller's pointers carry the lane's row / column and k = q
__device__ __forceinline__ f32x4 mm(const float* a, int as, const float* b, int bs, int n, f32x4 acc) {
    for (int s = 0; s < n; ++s) acc = mfma16(a[s * as], b[s * bs], acc);
    return acc;
}

// The LDS layout, in floats (it travels as a kernel argument): W shared, then `waves` areas of `per_wave` floats.
struct AiLds {
    int W, ldw, C16, wave0, per_wave;
    int X, Q, K, V, Z, T, S;                 // (T: one head's dQ, S: the row statistics)
    int ldx, ldc, waves, total;
};

struct AiArgs {
    const float *x, *wq, *wk, *wv, *wres;
    int B, F, D, A, H;
};

int round16(int v) { return (v + 15) & ~15; }

AiLds ai_lds(int F, int D, int A, int H, bool bwd, int waves) {
    AiLds L;
    const int F16 = round16(F), D16 = round16(D);
    L.C16 = round16(H * A);
    L.ldw = 4 * L.C16 + 17, L.ldx = D16 + 1, L.ldc = L.C16 + 1;
    L.W = 0, L.wave0 = D16 * L.ldw;
    int pw = 0;
    L.X = pw, pw += F16 * L.ldx;
    L.Q = pw, pw += F16 * L.ldc;
    L.K = pw, pw += F16 * L.ldc;
    L.V = pw, pw += F16 * L.ldc;
    L.Z = pw, pw += bwd ? F16 * L.ldc : 0;
    L.T = pw, pw += bwd ? F16 * kLdq : 0;
    L.S = pw, pw += bwd ? 3 * kStat : 0;
    L.per_wave = pw;
    L.waves = waves;
    L.total = L.wave0 + waves * pw;
    return L;
}

bool shape_ok(int F, int D, int A, int H) {
    return F >= RECALGO_AUTOINT_MIN_F && F <= RECALGO_AUTOINT_MAX_F && D >= RECALGO_AUTOINT_MIN_D && D <= RECALGO_AUTOINT_MAX_D &&
           (D & 3) == 0 && A >= RECALGO_AUTOINT_MIN_A && A <= RECALGO_AUTOINT_MAX_A && (A & 3) == 0 && H >= 1 &&
           H <= RECALGO_AUTOINT_MAX_H && H * A <= RECALGO_AUTOINT_MAX_HA;
}

// the most examples a workgroup serves at a time: 4, 2 or 1 waves, whichever the LDS of a workgroup holds (1 always fits)
int waves_for(int F, int D, int A, int H, bool bwd) {
    for (int w = kMaxWaves; w > 1; w >>= 1)
        if (sizeof(float) * (size_t)ai_lds(F, D, A, H, bwd, w).total <= kLdsMax) return w;
    return 1;
}

int groups_for(int B, int waves, int cap) {
    const int n = cdiv(B, waves);
    return n > cap ? cap : n;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------
// (ldx, ldc, ldw, C16: the layout's leading dimensions, handed down by value — the backward's are compile-time constants)
__device__ __forceinline__ void stage_shared(const AiArgs& a, const AiLds& L, float* sm, int ldw, int C16) {
    const int nthr = blockDim.x, HA = a.H * a.A, DA = a.D * a.A, HDA = a.H * DA;
    for (int i = threadIdx.x; i < L.total; i += nthr) sm[i] = 0.f;
    __syncthreads();
    for (int idx = threadIdx.x; idx < 3 * HDA; idx += nthr) {
        const int p = idx / HDA, rem = idx - p * HDA, h = rem / DA, d = (rem - h * DA) / a.A, c = h * a.A + rem % a.A;
        sm[L.W + d * ldw + p * C16 + c] = (p == 0 ? a.wq : (p == 1 ? a.wk : a.wv))[rem];
    }
    if (a.wres != nullptr)
        for (int idx = threadIdx.x; idx < a.D * HA; idx += nthr) sm[L.W + (idx / HA) * ldw + 3 * C16 + idx % HA] = a.wres[idx];
    __syncthreads();
}

// X <- the example's rows, then Q, K, V = X Wq, X Wk, X Wv over all heads at once
__device__ __forceinline__ void load_and_project(const AiArgs& a, const AiLds& L, const float* sm, float* mine, long long e, int lane,
                                                 int ldx, int ldc, int ldw, int C16) {
    const int r16 = lane & 15, q = lane >> 4;
    float* X = mine + L.X;
    const float* src = a.x + (size_t)e * a.F * a.D;
    for (int i = lane; i < a.F * a.D; i += 64) X[(i / a.D) * ldx + i % a.D] = src[i];
    wave_sync();
    const int nFT = (a.F + 15) >> 4, nCT = C16 >> 4, kD = a.D >> 2;
    for (int p = 0; p < 3; ++p) {
        float* dst = mine + (p == 0 ? L.Q : (p == 1 ? L.K : L.V));
        for (int ft = 0; ft < nFT; ++ft)
            for (int ct = 0; ct < nCT; ++ct) {
                const f32x4 acc = mm(X + (16 * ft + r16) * ldx + q, 4, sm + L.W + q * ldw + p * C16 + 16 * ct + r16, 4 * ldw,
                                     kD, zero4());
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[(16 * ft + 4 * q + i) * ldc + 16 * ct + r16] = acc[i];
            }
    }
    wave_sync();
}

// The softmax of head column `hc`, query tile ft, transposed: lane (r, q) gets P[f = 16 ft + r][j = 16 jt + 4 q + i] in p[jt][i]
// (0 for j >= F and for the key tiles past the last).
__device__ __forceinline__ void softmax_tile(const AiArgs& a, const AiLds& L, const float* Qs, const float* Ks, int hc, int ft,
                                             int lane, int ldc, f32x4 (&p)[kMaxJT], float& m, float& sum) {
    const int r16 = lane & 15, q = lane >> 4, nFT = (a.F + 15) >> 4, kA = a.A >> 2;
    m = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < kMaxJT; ++jt) {
        p[jt] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (jt < nFT) {
            p[jt] = mm(Ks + (16 * jt + r16) * ldc + hc + q, 4, Qs + (16 * ft + r16) * ldc + hc + q, 4, kA, zero4());
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (16 * jt + 4 * q + i >= a.F) p[jt][i] = -INFINITY;
                m = fmaxf(m, p[jt][i]);
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < kMaxJT; ++jt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[jt][i] = expf(p[jt][i] - m);                   // (key 0 is never masked: m is finite)
            sum += p[jt][i];
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
#pragma unroll
    for (int jt = 0; jt < kMaxJT; ++jt)
#pragma unroll
        for (int i = 0; i < 4; ++i) p[jt][i] = p[jt][i] / sum;
}

__global__ __launch_bounds__(64 * kMaxWaves) void autoint_fwd_kernel(AiArgs a, AiLds L, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int HA = a.H * a.A, nFT = (a.F + 15) >> 4, nAT = (a.A + 15) >> 4, kD = a.D >> 2;
    const int ldx = L.ldx, ldc = L.ldc, ldw = L.ldw, C16 = L.C16;
    stage_shared(a, L, sm, ldw, C16);
    float* mine = sm + L.wave0 + wave * L.per_wave;
    const float *X = mine + L.X, *Qs = mine + L.Q, *Ks = mine + L.K, *Vs = mine + L.V;
    for (long long e = (long long)blockIdx.x * L.waves + wave; e < a.B; e += (long long)gridDim.x * L.waves) {
        load_and_project(a, L, sm, mine, e, lane, ldx, ldc, ldw, C16);
        float* dst = y + (size_t)e * a.F * HA;
        for (int h = 0; h < a.H; ++h) {
            const int hc = h * a.A;
            for (int ft = 0; ft < nFT; ++ft) {
                f32x4 p[kMaxJT];
                float m, sum;
                softmax_tile(a, L, Qs, Ks, hc, ft, lane, ldc, p, m, sum);
                for (int at = 0; at < nAT; ++at) {
                    const int col = 16 * at + r16, cc = hc + (col < a.A ? col : a.A - 1);    // (a column past A is not stored)
                    f32x4 acc = zero4();
                    if (a.wres != nullptr)
                        acc = mm(X + (16 * ft + r16) * ldx + q, 4, sm + L.W + q * ldw + 3 * C16 + cc, 4 * ldw, kD, acc);
#pragma unroll
                    for (int jt = 0; jt < kMaxJT; ++jt)
                        if (jt < nFT) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc = mfma16(p[jt][i], Vs[(16 * jt + 4 * q + i) * ldc + cc], acc);
                        }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int f = 16 * ft + 4 * q + i;
                        if (f < a.F && col < a.A) dst[(size_t)f * HA + hc + col] = fmaxf(acc[i], 0.f);
                    }
                }
            }
        }
        wave_sync();                                         // (the next example overwrites X, Q, K, V)
    }
}

template <int DT, int CT, int NP>
__global__ __launch_bounds__(64 * kMaxWaves) void autoint_bwd_kernel(AiArgs a, AiLds L, const float* __restrict__ g_out,
                                                                      const float* __restrict__ y, float* __restrict__ dx,
                                                                      float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int AT = CT < 2 ? CT : 2;                      // 16-column tiles of a head: A <= 32 and A <= H A
    constexpr int PP = 4 / NP;                               // weight groups (Wq, Wk, Wv, Wres) a pass accumulates
    constexpr int C16 = 16 * CT, ldx = 16 * DT + 1, ldc = C16 + 1, ldw = 4 * C16 + 17;     // = ai_lds's
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int HA = a.H * a.A, nFT = (a.F + 15) >> 4, nAT = (a.A + 15) >> 4, kA = a.A >> 2, kF = (a.F + 3) >> 2, kC = HA >> 2;
    const bool res = a.wres != nullptr;
    stage_shared(a, L, sm, ldw, C16);
    float* mine = sm + L.wave0 + wave * L.per_wave;
    float *X = mine + L.X, *Qs = mine + L.Q, *Ks = mine + L.K, *Vs = mine + L.V, *Zs = mine + L.Z, *DQ = mine + L.T, *St = mine + L.S;

    const int HDA = a.H * a.D * a.A, n_row = 3 * HDA + (res ? a.D * HA : 0);
    float* prow = partials + (size_t)blockIdx.x * n_row;
    for (int pass = 0; pass < NP; ++pass) {
    f32x4 dw[DT][PP * CT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int c = 0; c < PP * CT; ++c) dw[dt][c] = zero4();

    for (long long e = (long long)blockIdx.x * L.waves + wave; e < a.B; e += (long long)gridDim.x * L.waves) {
        {   // dZ = g [y > 0]
            const float *gs = g_out + (size_t)e * a.F * HA, *ys = y + (size_t)e * a.F * HA;
            for (int i = lane; i < a.F * HA; i += 64) Zs[(i / HA) * ldc + i % HA] = ys[i] > 0.f ? gs[i] : 0.f;
        }
        load_and_project(a, L, sm, mine, e, lane, ldx, ldc, ldw, C16);
        for (int h = 0; h < a.H; ++h) {
            const int hc = h * a.A;
            // by query tile: the softmax's row statistics, rs = rowsum(P * dP), and dQ = dS K (kept in DQ: Q is still read)
            for (int ft = 0; ft < nFT; ++ft) {
                f32x4 p[kMaxJT], ds[kMaxJT];
                float m, sum;
                softmax_tile(a, L, Qs, Ks, hc, ft, lane, ldc, p, m, sum);
                float rs = 0.f;
#pragma unroll
                for (int jt = 0; jt < kMaxJT; ++jt) {
                    ds[jt] = zero4();
                    if (jt < nFT) {                          // dP^T in the layout of P
                        ds[jt] = mm(Vs + (16 * jt + r16) * ldc + hc + q, 4, Zs + (16 * ft + r16) * ldc + hc + q, 4, kA, zero4());
#pragma unroll
                        for (int i = 0; i < 4; ++i) rs = fmaf(p[jt][i], ds[jt][i], rs);
                    }
                }
                rs += __shfl_xor(rs, 16, 64);
                rs += __shfl_xor(rs, 32, 64);
                if (q == 0) St[16 * ft + r16] = m, St[kStat + 16 * ft + r16] = sum, St[2 * kStat + 16 * ft + r16] = rs;
#pragma unroll
                for (int jt = 0; jt < kMaxJT; ++jt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) ds[jt][i] = p[jt][i] * (ds[jt][i] - rs);
#pragma unroll
                for (int at = 0; at < AT; ++at)
                    if (at < nAT) {
                        const int col = 16 * at + r16, cc = hc + (col < a.A ? col : a.A - 1);
                        f32x4 dq = zero4();
#pragma unroll
                        for (int jt = 0; jt < kMaxJT; ++jt)
                            if (jt < nFT) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) dq = mfma16(ds[jt][i], Ks[(16 * jt + 4 * q + i) * ldc + cc], dq);
                            }
#pragma unroll
                        for (int i = 0; i < 4; ++i) DQ[(16 * ft + 4 * q + i) * kLdq + col] = dq[i];
                    }
            }
            wave_sync();
            // by key tile: P and dS in the other orientation (lane (r, q): f = 4 q + i, j = r) from the statistics, so that
            // dK = dS^T Q and dV = P^T dZ of the tile need four accumulators; they take the place of the tile's K and V
            for (int jt = 0; jt < nFT; ++jt) {
                f32x4 dk[AT], dv[AT];
#pragma unroll
                for (int at = 0; at < AT; ++at) dk[at] = zero4(), dv[at] = zero4();
                const bool key = 16 * jt + r16 < a.F;
                for (int ft = 0; ft < nFT; ++ft) {
                    const f32x4 s2 = mm(Qs + (16 * ft + r16) * ldc + hc + q, 4, Ks + (16 * jt + r16) * ldc + hc + q, 4, kA, zero4());
                    const f32x4 dp = mm(Zs + (16 * ft + r16) * ldc + hc + q, 4, Vs + (16 * jt + r16) * ldc + hc + q, 4, kA, zero4());
                    float p2[4], ds2[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int f = 16 * ft + 4 * q + i;
                        p2[i] = key ? expf(s2[i] - St[f]) / St[kStat + f] : 0.f;
                        ds2[i] = p2[i] * (dp[i] - St[2 * kStat + f]);
                    }
#pragma unroll
                    for (int at = 0; at < AT; ++at)
                        if (at < nAT) {
                            const int col = 16 * at + r16, cc = hc + (col < a.A ? col : a.A - 1);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                dv[at] = mfma16(p2[i], Zs[(16 * ft + 4 * q + i) * ldc + cc], dv[at]);
                                dk[at] = mfma16(ds2[i], Qs[(16 * ft + 4 * q + i) * ldc + cc], dk[at]);
                            }
                        }
                }
                wave_sync();                                 // (every lane is done with the tile's K and V rows)
#pragma unroll
                for (int at = 0; at < AT; ++at)
                    if (at < nAT) {
                        const int col = 16 * at + r16;
                        if (col < a.A) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                Ks[(16 * jt + 4 * q + i) * ldc + hc + col] = dk[at][i];
                                Vs[(16 * jt + 4 * q + i) * ldc + hc + col] = dv[at][i];
                            }
                        }
                    }
            }
            wave_sync();
            // dQ takes the place of this head's Q
            for (int i = lane; i < 16 * nFT * a.A; i += 64) Qs[(i / a.A) * ldc + hc + i % a.A] = DQ[(i / a.A) * kLdq + i % a.A];
            wave_sync();
        }
        wave_sync();
        // dx = dQ Wq^T + dK Wk^T + dV Wv^T (+ dZ Wres^T), over the head-major columns c
        float* dst = dx + (size_t)e * a.F * a.D;
        for (int ft = 0; pass == 0 && ft < nFT; ++ft)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                f32x4 acc = zero4();
                for (int p = 0; p < (res ? 4 : 3); ++p) {
                    const float* G = p == 0 ? Qs : (p == 1 ? Ks : (p == 2 ? Vs : Zs));
                    acc = mm(G + (16 * ft + r16) * ldc + q, 4, sm + L.W + (16 * dt + r16) * ldw + p * C16 + q, 4, kC, acc);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = 16 * ft + 4 * q + i, d = 16 * dt + r16;
                    if (f < a.F && d < a.D) dst[(size_t)f * a.D + d] = acc[i];
                }
            }
        // dW += X^T [dQ | dK | dV | dZ]  (the rows F .. 4 kF of every operand are zero): a k-step's operands feed every tile
        for (int s = 0; s < kF; ++s) {
            float xa[DT], gb[PP * CT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) xa[dt] = X[(4 * s + q) * ldx + 16 * dt + r16];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                const int p = pass * PP + pp;
                const float* G = p == 0 ? Qs : (p == 1 ? Ks : (p == 2 ? Vs : Zs));      // (without Wres dZ's product is not stored)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) gb[pp * CT + ct] = G[(4 * s + q) * ldc + 16 * ct + r16];
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int c = 0; c < PP * CT; ++c) dw[dt][c] = mfma16(xa[dt], gb[c], dw[dt][c]);
        }
        wave_sync();                                         // (the next example overwrites X, Q, K, V, dZ)
    }

    // the pass's part of the workgroup's partial row [dWq | dWk | dWv | dWres]: the waves add theirs in wave order (a wave without
    // an example adds zeros).  An element is written and read by the same lane of every wave; wave w passes w barriers, adds,
    // and passes the remaining ones, so every wave meets `waves` barriers and the adds are ordered.
    for (int turn = 0; turn < wave; ++turn) __syncthreads();
#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
        const int p = pass * PP + pp;
        if (p == 3 && !res) continue;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int c = 16 * ct + r16;
            float* col = prow + (p < 3 ? p * HDA + (c / a.A) * a.D * a.A + c % a.A : 3 * HDA + c);
            const int step = p < 3 ? a.A : HA;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = 16 * dt + 4 * q + i;
                    if (d < a.D && c < HA) {
                        const float v = dw[dt][pp * CT + ct][i];
                        col[d * step] = wave == 0 ? v : col[d * step] + v;
                    }
                }
                asm volatile("" ::: "memory");               // (a tile at a time)
            }
        }
    }
    for (int turn = wave; turn < L.waves; ++turn) __syncthreads();
    }
}

// the accumulators of dW are 16 DT CT registers in one pass: from nine tile pairs on the examples are walked twice, [dWq | dWk]
// then [dWv | dWres] (dx is written in the first pass), which halves them — one pass there needs scratch
template <int DT, int CT>
hipError_t launch_bwd(dim3 grid, dim3 block, size_t lds, hipStream_t st, const AiArgs& a, const AiLds& L, const float* g,
                      const float* y, float* dx, float* ws) {
    return launch_lds<autoint_bwd_kernel<DT, CT, (DT * CT >= 9 ? 2 : 1)>>(grid, block, lds, st, a, L, g, y, dx, ws);
}

typedef hipError_t (*bwd_launcher)(dim3, dim3, size_t, hipStream_t, const AiArgs&, const AiLds&, const float*, const float*,
                                   float*, float*);
// [16-row tiles of D - 1][16-column tiles of H A - 1]
const bwd_launcher kBwd[4][4] = {{launch_bwd<1, 1>, launch_bwd<1, 2>, launch_bwd<1, 3>, launch_bwd<1, 4>},
                                 {launch_bwd<2, 1>, launch_bwd<2, 2>, launch_bwd<2, 3>, launch_bwd<2, 4>},
                                 {launch_bwd<3, 1>, launch_bwd<3, 2>, launch_bwd<3, 3>, launch_bwd<3, 4>},
                                 {launch_bwd<4, 1>, launch_bwd<4, 2>, launch_bwd<4, 3>, launch_bwd<4, 4>}};

int64_t row_floats(int D, int A, int H, bool res) { return (int64_t)(res ? 4 : 3) * H * D * A; }

}  // namespace

RECALGO_EXPORT int recalgo_autoint_abi_version(void) { return RECALGO_AUTOINT_ABI_VERSION; }

RECALGO_EXPORT int recalgo_autoint_supported(int F, int D, int A, int H) { return shape_ok(F, D, A, H) ? 1 : 0; }

RECALGO_EXPORT int recalgo_autoint_bwd_partial_rows(int B, int F, int D, int A, int H) {
    if (B < 1 || !shape_ok(F, D, A, H)) return 0;
    return groups_for(B, waves_for(F, D, A, H, true), kBwdGrid);
}

RECALGO_EXPORT int64_t recalgo_autoint_bwd_workspace_bytes(int B, int F, int D, int A, int H, int has_res) {
    return (int64_t)sizeof(float) * recalgo_autoint_bwd_partial_rows(B, F, D, A, H) * row_floats(D, A, H, has_res != 0);
}

RECALGO_EXPORT int recalgo_autoint_layer_fwd(const float* x, const float* wq, const float* wk, const float* wv, const float* wres,
                                             int B, int F, int D, int A, int H, float* y, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(F, D, A, H));
    RECALGO_REQUIRE(x && wq && wk && wv && y);
    RECALGO_REQUIRE(aligned_to<4>(x, wq, wk, wv, wres, y));
    const int waves = waves_for(F, D, A, H, false);
    const AiLds L = ai_lds(F, D, A, H, false, waves);
    const AiArgs a = {x, wq, wk, wv, wres, B, F, D, A, H};
    RECALGO_CHECK(launch_lds<autoint_fwd_kernel>(dim3(groups_for(B, waves, kFwdGrid)), dim3(64 * waves),
                                                 sizeof(float) * (size_t)L.total, as_stream(stream), a, L, y));
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_autoint_layer_bwd(const float* g, const float* x, const float* y, const float* wq, const float* wk,
                                             const float* wv, const float* wres, int B, int F, int D, int A, int H, float* dx,
                                             float* dwq, float* dwk, float* dwv, float* dwres, void* workspace,
                                             recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(F, D, A, H));
    RECALGO_REQUIRE(g && x && y && wq && wk && wv && dx && dwq && dwk && dwv && workspace);
    RECALGO_REQUIRE((wres == nullptr) == (dwres == nullptr));
    RECALGO_REQUIRE(aligned_to<4>(g, x, y, wq, wk, wv, wres, dx, dwq, dwk, dwv, dwres) && aligned_to<4>(workspace));
    const int waves = waves_for(F, D, A, H, true);
    const AiLds L = ai_lds(F, D, A, H, true, waves);
    const AiArgs a = {x, wq, wk, wv, wres, B, F, D, A, H};
    const int rows = groups_for(B, waves, kBwdGrid);
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(workspace);
    RECALGO_CHECK(kBwd[(D + 15) / 16 - 1][(H * A + 15) / 16 - 1](dim3(rows), dim3(64 * waves), sizeof(float) * (size_t)L.total, st, a,
                                                                 L, g, y, dx, ws));
    const int HDA = H * D * A;
    float* const outs[4] = {dwq, dwk, dwv, dwres};
    const int starts[5] = {0, HDA, 2 * HDA, 3 * HDA, 3 * HDA + D * H * A};
    return recalgo_slabs::launch_colsums(ws, rows, wres ? 4 : 3, outs, starts, st);
}
