// AFM's attention network (include/recalgo_afm.h; algorithm/AFM/afm.py:162-188), one kernel each way.
//
// One wave per example, up to four waves per workgroup.  The example's [F][K] block lies in LDS (row stride K + 1); the pairs
// (i < j, row-major) are walked in tiles of 16, the last one masked.  A tile's pair products are formed in registers as an
// operand of v_mfma_f32_16x16x4_f32: lane l = (r, q) = (l & 15, l >> 4) holds pair r's elements k = 4 s + q, s = 0 .. K/4 - 1.
// w is read once per workgroup into LDS in operand order (wB: the value lane l needs at k-step s and column tile c is at
// ((s * nCT + c) * 64 + l), w[4 s + q][16 c + r]), so the SAME two registers give both orientations of z = pair w:
//   z  = mfma(pairs, wB): lane holds pairs 4 q + reg, column 16 c + r          ("row form": sums over a column's pairs are in-lane)
//   zT = mfma(wB, pairs): lane holds pair r, columns 16 c + 4 q + reg          ("column form": dz is an A operand as it stands)
// The forward uses the row form: bias, ReLU and `* h` on the accumulator, a score summed over t in double (in-lane over the
// column tiles, then a butterfly over the 16 lanes of a row).  The softmax over the example's P scores is shifted by its maximum.
//
// The backward takes the softmax from the saved scores, so it walks the tiles once.  Per tile and column tile it recomputes
// z in both forms (an MFMA's k-order is free: the products below pair lane group q with the element the lane ALREADY holds,
// so no value crosses lanes or goes through LDS):
//   dw   += pair^T dz        A = pair products (pair 4 q + s, k = 16 kt + r), B = dz in row form, register s
//   dpair = dz w^T           A = dz in column form, register s, B = wT (w[16 kt + r][16 c + 4 q + s], a second LDS copy)
// db and dh are in-lane sums of the row form.  dw, db, dh stay in registers over all tiles and examples of the wave; at the end
// the waves of a workgroup add them in wave order into ONE partial row [dw | db | dh] (LDS, then global), and
// recalgo_slabs::launch_colsums sums the rows.  d_fields: the dpair tile goes to a 16-row LDS tile, then lane (k, side) walks
// its 16 rows in order: side 0 adds dpair_(i,j) * e_j to dF[i], side 1 dpair_(i,j) * e_i to dF[j] — in the row-major pair
// order that is field order of the partner for every row of dF, with no atomics.  Nothing depends on B or on which wave or
// workgroup serves an example.
#include "common.h"
#include "slab_sum.h"
#include "../../include/recalgo_afm.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxWaves = 4;
constexpr int kMaxCT = RECALGO_AFM_MAX_T / 16;
constexpr int kFwdGrid = 4096;
constexpr int kBwdGrid = RECALGO_AFM_MAX_PARTIAL_ROWS;

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The LDS layout, in floats (it travels as a kernel argument).  Shared by the workgroup: wB, wT (backward), bias, h, the pair
// table; then `waves` areas of `per_wave` floats: E, dF, sc, ds, dp, g at the offsets below.
struct AfmLds {
    int wB, wT, bias, hh, pairs, wave0, per_wave;
    int E, dF, sc, ds, dp, g;
    int ld, dpld, P, P16, waves, total;
};

struct AfmArgs {
    const float *fields, *w, *b, *h;
    int B, F, t;
};

int round16(int v) { return (v + 15) & ~15; }

AfmLds afm_lds(int F, int K, int t, bool bwd, int waves) {
    AfmLds L;
    const int KT = (K + 15) / 16;
    L.P = F * (F - 1) / 2, L.P16 = round16(L.P);
    L.ld = K + 1, L.dpld = 16 * KT + 1;
    int at = 0;
    L.wB = at, at += K * t;
    L.wT = at, at += bwd ? 16 * KT * t : 0;          // (wB and wT together hold the K t + 2 t floats of the partial row)
    L.bias = at, at += t;
    L.hh = at, at += t;
    L.pairs = at, at += L.P16;
    L.wave0 = at;
    int pw = 0;
    L.E = pw, pw += round4(F * L.ld);
    L.dF = pw, pw += bwd ? round4(F * L.ld) : 0;
    L.sc = pw, pw += L.P16;
    L.ds = pw, pw += bwd ? L.P16 : 0;
    L.dp = pw, pw += bwd ? round4(16 * L.dpld) : 0;
    L.g = pw, pw += bwd ? RECALGO_AFM_MAX_K : 0;
    L.per_wave = pw;
    L.waves = waves;
    L.total = at + waves * pw;
    return L;
}

bool shape_ok(int F, int K, int t) {
    return F >= 2 && F <= RECALGO_AFM_MAX_F && K >= 4 && K <= RECALGO_AFM_MAX_K && (K & 3) == 0 && t >= 16 &&
           t <= RECALGO_AFM_MAX_T && (t & 15) == 0;
}

// the most examples a workgroup serves at a time: 4, 2 or 1 waves, whichever the LDS of a workgroup holds (1 always fits)
int waves_for(int F, int K, int t, bool bwd) {
    for (int w = kMaxWaves; w > 1; w >>= 1)
        if (sizeof(float) * (size_t)afm_lds(F, K, t, bwd, w).total <= kLdsMax) return w;
    return 1;
}

int groups_for(int B, int waves, int cap) {
    const int n = cdiv(B, waves);
    return n > cap ? cap : n;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void stage_shared(const AfmArgs& a, const AfmLds& L, float* sm, bool bwd) {
    constexpr int KT = (K + 15) / 16;
    const int t = a.t, nCT = t >> 4, nthr = blockDim.x;
    for (int idx = threadIdx.x; idx < K * t; idx += nthr) {
        const int l = idx & 63, sc = idx >> 6, c = sc % nCT, s = sc / nCT;
        sm[L.wB + idx] = a.w[(4 * s + (l >> 4)) * t + 16 * c + (l & 15)];
    }
    if (bwd) {
        for (int idx = threadIdx.x; idx < 16 * KT * t; idx += nthr) {
            const int l = idx & 63, r = idx >> 6, kt = r % KT, r2 = r / KT, s = r2 & 3, c = r2 >> 2;
            const int k = 16 * kt + (l & 15), col = 16 * c + 4 * (l >> 4) + s;
            sm[L.wT + idx] = k < K ? a.w[k * t + col] : 0.f;
        }
    }
    for (int i = threadIdx.x; i < t; i += nthr) sm[L.bias + i] = a.b[i], sm[L.hh + i] = a.h[i];
    int* tab = reinterpret_cast<int*>(sm + L.pairs);
    for (int i = 0; i + 1 < a.F; ++i) {
        const int base = i * (2 * a.F - i - 1) / 2;
        for (int j = i + 1 + threadIdx.x; j < a.F; j += nthr) tab[base + j - i - 1] = i | (j << 8);
    }
    for (int p = L.P + threadIdx.x; p < L.P16; p += nthr) tab[p] = 0 | (1 << 8);        // (masked rows: a valid pair, F >= 2)
}

template <int K>
__device__ __forceinline__ void load_example(const float* fields, long long e, int F, const AfmLds& L, float* E, int lane) {
    const float* src = fields + (size_t)e * F * K;
    for (int i = lane; i < F * K; i += 64) E[(i / K) * L.ld + i % K] = src[i];
}

// the tile's pair products as the 16-row operand: lane (r, q) holds pair p0 + r, element 4 s + q
template <int K>
__device__ __forceinline__ void pair_operand(const float* E, const int* tab, const AfmLds& L, int p0, int lane, float (&A)[K / 4]) {
    const int p = p0 + (lane & 15), ij = tab[p], q = lane >> 4;
    const float *ei = E + (ij & 255) * L.ld + q, *ej = E + (ij >> 8) * L.ld + q;
#pragma unroll
    for (int s = 0; s < K / 4; ++s) A[s] = p < L.P ? ei[4 * s] * ej[4 * s] : 0.f;
}

// sc[0 .. P) -> softmax(sc), shifted by its maximum; sc[P .. P16) -> 0.  A lane touches only the elements p = lane (mod 64).
__device__ __forceinline__ void softmax_inplace(float* sc, const AfmLds& L, int lane) {
    float m = -INFINITY;
    for (int p = lane; p < L.P; p += 64) m = fmaxf(m, sc[p]);
    m = wave_max(m);
    float sum = 0.f;
    for (int p = lane; p < L.P; p += 64) {
        const float ex = expf(sc[p] - m);
        sc[p] = ex, sum += ex;
    }
    sum = wave_sum(sum);
    for (int p = lane; p < L.P; p += 64) sc[p] = sc[p] / sum;
    for (int p = L.P + lane; p < L.P16; p += 64) sc[p] = 0.f;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int K>
__global__ __launch_bounds__(64 * kMaxWaves) void afm_fwd_kernel(AfmArgs a, AfmLds L, float* __restrict__ out,
                                                                  float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int KP = K <= 4 ? 4 : (K <= 8 ? 8 : (K <= 16 ? 16 : 32));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int nCT = a.t >> 4;
    stage_shared<K>(a, L, sm, false);
    __syncthreads();
    const int* tab = reinterpret_cast<const int*>(sm + L.pairs);
    float* mine = sm + L.wave0 + wave * L.per_wave;
    float *E = mine + L.E, *sc = mine + L.sc;
    for (long long e = (long long)blockIdx.x * L.waves + wave; e < a.B; e += (long long)gridDim.x * L.waves) {
        load_example<K>(a.fields, e, a.F, L, E, lane);
        wave_sync();
        for (int p0 = 0; p0 < L.P; p0 += 16) {
            float A[K / 4];
            pair_operand<K>(E, tab, L, p0, lane, A);
            double part[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < nCT; c += 2) {              // two column tiles at a time: two independent accumulator chains
                const bool two = c + 1 < nCT;
                f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < K / 4; ++s) {
                    z0 = mfma16(A[s], sm[L.wB + (s * nCT + c) * 64 + lane], z0);
                    if (two) z1 = mfma16(A[s], sm[L.wB + (s * nCT + c + 1) * 64 + lane], z1);
                }
                const double h0 = (double)sm[L.hh + 16 * c + r16];
                const float b0 = sm[L.bias + 16 * c + r16];
#pragma unroll
                for (int i = 0; i < 4; ++i) part[i] = fma((double)fmaxf(z0[i] + b0, 0.f), h0, part[i]);
                if (two) {
                    const double h1 = (double)sm[L.hh + 16 * c + 16 + r16];
                    const float b1 = sm[L.bias + 16 * c + 16 + r16];
#pragma unroll
                    for (int i = 0; i < 4; ++i) part[i] = fma((double)fmaxf(z1[i] + b1, 0.f), h1, part[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) part[i] += __shfl_xor(part[i], o, 64);
            }
            if (r16 < 4) {                                   // lane (r, q), r < 4, stores pair p0 + 4 q + r
                const float s = (float)(r16 == 0 ? part[0] : (r16 == 1 ? part[1] : (r16 == 2 ? part[2] : part[3])));
                const int p = p0 + 4 * q + r16;
                if (p < L.P) {
                    sc[p] = s;
                    if (scores != nullptr) scores[(size_t)e * L.P + p] = s;
                }
            }
        }
        wave_sync();
        softmax_inplace(sc, L, lane);
        wave_sync();
        // out[k] = sum_p a_p pair_p[k]: lane (k, grp) adds the pairs grp, grp + G, .. in order, then the groups in a butterfly
        constexpr int G = 64 / KP;
        const int k = lane & (KP - 1), grp = lane / KP;
        double o = 0.0;
        if (k < K) {
            for (int p = grp; p < L.P; p += G) {
                const int ij = tab[p];
                o = fma((double)sc[p], (double)(E[(ij & 255) * L.ld + k] * E[(ij >> 8) * L.ld + k]), o);
            }
        }
#pragma unroll
        for (int off = KP; off < 64; off <<= 1) o += __shfl_xor(o, off, 64);
        if (grp == 0 && k < K) out[(size_t)e * K + k] = (float)o;
        wave_sync();                                         // (the next example overwrites E and sc)
    }
}

template <int K>
__global__ __launch_bounds__(64 * kMaxWaves) void afm_bwd_kernel(AfmArgs a, AfmLds L, const float* __restrict__ g_out,
                                                                  const float* __restrict__ scores, float* __restrict__ d_fields,
                                                                  float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int KT = (K + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int t = a.t, nCT = t >> 4;
    stage_shared<K>(a, L, sm, true);
    __syncthreads();
    const int* tab = reinterpret_cast<const int*>(sm + L.pairs);
    float* mine = sm + L.wave0 + wave * L.per_wave;
    float *E = mine + L.E, *dF = mine + L.dF, *sc = mine + L.sc, *ds = mine + L.ds, *dp = mine + L.dp, *gk = mine + L.g;

    f32x4 dwacc[KT][kMaxCT];
    float dbacc[kMaxCT], dhacc[kMaxCT];
#pragma unroll
    for (int c = 0; c < kMaxCT; ++c) {
        dbacc[c] = 0.f, dhacc[c] = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) dwacc[kt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (long long e = (long long)blockIdx.x * L.waves + wave; e < a.B; e += (long long)gridDim.x * L.waves) {
        load_example<K>(a.fields, e, a.F, L, E, lane);
        if (lane < K) gk[lane] = g_out[(size_t)e * K + lane];
        for (int p = lane; p < L.P; p += 64) sc[p] = scores[(size_t)e * L.P + p];
        for (int i = lane; i < a.F * L.ld; i += 64) dF[i] = 0.f;
        wave_sync();
        softmax_inplace(sc, L, lane);                        // sc = a
        // da_p = g . pair_p;  ds_p = a_p (da_p - sum_q a_q da_q)      (a lane keeps to its own p = lane mod 64: no barrier between)
        double sa = 0.0;
        for (int p = lane; p < L.P; p += 64) {
            const int ij = tab[p];
            const float *ei = E + (ij & 255) * L.ld, *ej = E + (ij >> 8) * L.ld;
            float da = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) da = fmaf(gk[k], ei[k] * ej[k], da);
            ds[p] = da;
            sa = fma((double)sc[p], (double)da, sa);
        }
        sa = wave_sum_f64(sa);
        for (int p = lane; p < L.P; p += 64) ds[p] = (float)((double)sc[p] * ((double)ds[p] - sa));
        for (int p = L.P + lane; p < L.P16; p += 64) ds[p] = 0.f;
        wave_sync();

        for (int p0 = 0; p0 < L.P; p0 += 16) {
            float A[K / 4];
            pair_operand<K>(E, tab, L, p0, lane, A);
            // the dw product's 16-row operand: pair p0 + 4 q + s, element 16 kt + r
            float PT[KT][4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int p = p0 + 4 * q + s, ij = tab[p];
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    const int k = 16 * kt + r16;
                    PT[kt][s] = (p < L.P && k < K) ? E[(ij & 255) * L.ld + k] * E[(ij >> 8) * L.ld + k] : 0.f;
                }
            }
            const float4 dsr = *reinterpret_cast<const float4*>(ds + p0 + 4 * q);     // row form: pairs 4 q + reg
            const float dsT = ds[p0 + r16];                                            // column form: pair r
            f32x4 dpacc[KT][2];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) dpacc[kt][0] = f32x4{0.f, 0.f, 0.f, 0.f}, dpacc[kt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < kMaxCT; ++c) {
                if (c < nCT) {
                    f32x4 z = {0.f, 0.f, 0.f, 0.f}, zT = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < K / 4; ++s) {
                        const float wv = sm[L.wB + (s * nCT + c) * 64 + lane];
                        z = mfma16(A[s], wv, z);
                        zT = mfma16(wv, A[s], zT);
                    }
                    const float bc = sm[L.bias + 16 * c + r16], hc = sm[L.hh + 16 * c + r16];
                    const float dsv[4] = {dsr.x, dsr.y, dsr.z, dsr.w};
                    float dz[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float zz = z[i] + bc;
                        dz[i] = zz > 0.f ? dsv[i] * hc : 0.f;
                        dbacc[c] += dz[i];
                        dhacc[c] = fmaf(dsv[i], fmaxf(zz, 0.f), dhacc[c]);
                    }
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int s = 0; s < 4; ++s) dwacc[kt][c] = mfma16(PT[kt][s], dz[s], dwacc[kt][c]);
                    const float4 bT = *reinterpret_cast<const float4*>(sm + L.bias + 16 * c + 4 * q);
                    const float4 hT = *reinterpret_cast<const float4*>(sm + L.hh + 16 * c + 4 * q);
                    const float bTv[4] = {bT.x, bT.y, bT.z, bT.w}, hTv[4] = {hT.x, hT.y, hT.z, hT.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const float dzT = zT[s] + bTv[s] > 0.f ? dsT * hTv[s] : 0.f;
#pragma unroll
                        for (int kt = 0; kt < KT; ++kt)
                            dpacc[kt][c & 1] = mfma16(dzT, sm[L.wT + ((c * 4 + s) * KT + kt) * 64 + lane], dpacc[kt][c & 1]);
                    }
                }
            }
            // dz w^T of the tile -> dp[pair 4 q + reg][k = 16 kt + r]
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int i = 0; i < 4; ++i) dp[(4 * q + i) * L.dpld + 16 * kt + r16] = dpacc[kt][0][i] + dpacc[kt][1][i];
            wave_sync();
            {   // lane (k, side): dF[i] += dpair * e_j (side 0), dF[j] += dpair * e_i (side 1), the tile's pairs in order
                const int k = lane & 31, side = lane >> 5;
                const float gv = k < K ? gk[k] : 0.f;
                const int rows = L.P - p0 < 16 ? L.P - p0 : 16;
                for (int r = 0; r < rows; ++r) {
                    if (k < K) {
                        const int ij = tab[p0 + r], i = ij & 255, j = ij >> 8;
                        const float v = fmaf(sc[p0 + r], gv, dp[r * L.dpld + k]);
                        const int f = side ? j : i, o = side ? i : j;
                        dF[f * L.ld + k] = fmaf(v, E[o * L.ld + k], dF[f * L.ld + k]);
                    }
                    wave_sync();                             // (pair r + 1 may add to the row another lane has just written)
                }
            }
            wave_sync();                                     // (the next tile overwrites dp)
        }
        float* dst = d_fields + (size_t)e * a.F * K;
        for (int i = lane; i < a.F * K; i += 64) dst[i] = dF[(i / K) * L.ld + i % K];
        wave_sync();                                         // (the next example overwrites E, dF, sc, ds, g)
    }

    // the workgroup's partial row [dw | db | dh], the waves added in wave order (a wave without an example adds zeros)
    __syncthreads();                                         // (every wave is done with wB / wT: the row takes their place)
    float* row = sm;
    const int n_row = K * t + 2 * t;
    for (int wv = 0; wv < L.waves; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int c = 0; c < kMaxCT; ++c) {
                if (c < nCT) {
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int k = 16 * kt + 4 * q + i;
                            if (k < K) {
                                float* at = row + k * t + 16 * c + r16;
                                *at = wv == 0 ? dwacc[kt][c][i] : *at + dwacc[kt][c][i];
                            }
                        }
                    // the four lane groups hold the sums of the pairs 4 q + reg: added in group order
                    const float b0 = __shfl(dbacc[c], r16, 64), b1 = __shfl(dbacc[c], 16 + r16, 64);
                    const float b2 = __shfl(dbacc[c], 32 + r16, 64), b3 = __shfl(dbacc[c], 48 + r16, 64);
                    const float h0 = __shfl(dhacc[c], r16, 64), h1 = __shfl(dhacc[c], 16 + r16, 64);
                    const float h2 = __shfl(dhacc[c], 32 + r16, 64), h3 = __shfl(dhacc[c], 48 + r16, 64);
                    if (q == 0) {
                        const float db = (b0 + b1) + (b2 + b3), dh = (h0 + h1) + (h2 + h3);
                        float *atb = row + K * t + 16 * c + r16, *ath = atb + t;
                        *atb = wv == 0 ? db : *atb + db;
                        *ath = wv == 0 ? dh : *ath + dh;
                    }
                }
            }
        }
        __syncthreads();
    }
    float* prow = partials + (size_t)blockIdx.x * n_row;
    for (int i = threadIdx.x; i < n_row; i += blockDim.x) prow[i] = row[i];
}

// launch_lds raises the dynamic-LDS allowance of the instantiation it launches (K is one of 4, 8, .., 32: shape_ok)
#define AFM_LAUNCH(KERNEL, K, grid, block, lds, st, ...)                                                  \
    RECALGO_CHECK((K) == 4    ? launch_lds<KERNEL<4>>(grid, block, lds, st, __VA_ARGS__)                   \
                  : (K) == 8  ? launch_lds<KERNEL<8>>(grid, block, lds, st, __VA_ARGS__)                   \
                  : (K) == 12 ? launch_lds<KERNEL<12>>(grid, block, lds, st, __VA_ARGS__)                  \
                  : (K) == 16 ? launch_lds<KERNEL<16>>(grid, block, lds, st, __VA_ARGS__)                  \
                  : (K) == 20 ? launch_lds<KERNEL<20>>(grid, block, lds, st, __VA_ARGS__)                  \
                  : (K) == 24 ? launch_lds<KERNEL<24>>(grid, block, lds, st, __VA_ARGS__)                  \
                  : (K) == 28 ? launch_lds<KERNEL<28>>(grid, block, lds, st, __VA_ARGS__)                  \
                              : launch_lds<KERNEL<32>>(grid, block, lds, st, __VA_ARGS__))

}  // namespace

RECALGO_EXPORT int recalgo_afm_abi_version(void) { return RECALGO_AFM_ABI_VERSION; }

RECALGO_EXPORT int recalgo_afm_supported(int F, int K, int t) { return shape_ok(F, K, t) ? 1 : 0; }

RECALGO_EXPORT int recalgo_afm_bwd_partial_rows(int B, int F, int K, int t) {
    if (B < 1 || !shape_ok(F, K, t)) return 0;
    return groups_for(B, waves_for(F, K, t, true), kBwdGrid);
}

RECALGO_EXPORT int64_t recalgo_afm_bwd_workspace_bytes(int B, int F, int K, int t) {
    return (int64_t)sizeof(float) * recalgo_afm_bwd_partial_rows(B, F, K, t) * ((int64_t)K * t + 2 * t);
}

RECALGO_EXPORT int recalgo_afm_attention_fwd(const float* fields, const float* w, const float* b, const float* h, int B, int F,
                                             int K, int t, float* out, float* scores, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(F, K, t));
    RECALGO_REQUIRE(fields && w && b && h && out);
    RECALGO_REQUIRE(aligned_to<4>(fields, w, b, h, out, scores));
    const int waves = waves_for(F, K, t, false);
    const AfmLds L = afm_lds(F, K, t, false, waves);
    const AfmArgs a = {fields, w, b, h, B, F, t};
    AFM_LAUNCH(afm_fwd_kernel, K, dim3(groups_for(B, waves, kFwdGrid)), dim3(64 * waves), sizeof(float) * (size_t)L.total,
               as_stream(stream), a, L, out, scores);
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_afm_attention_bwd(const float* g, const float* fields, const float* w, const float* b, const float* h,
                                             const float* scores, int B, int F, int K, int t, float* d_fields, float* dw,
                                             float* db, float* dh, void* workspace, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(F, K, t));
    RECALGO_REQUIRE(g && fields && w && b && h && scores && d_fields && dw && db && dh && workspace);
    RECALGO_REQUIRE(aligned_to<4>(g, fields, w, b, h, scores, d_fields, dw, db, dh) && aligned_to<4>(workspace));
    const int waves = waves_for(F, K, t, true);
    const AfmLds L = afm_lds(F, K, t, true, waves);
    const AfmArgs a = {fields, w, b, h, B, F, t};
    const int rows = groups_for(B, waves, kBwdGrid);
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(workspace);
    AFM_LAUNCH(afm_bwd_kernel, K, dim3(rows), dim3(64 * waves), sizeof(float) * (size_t)L.total, st, a, L, g, scores, d_fields, ws);
    float* const outs[3] = {dw, db, dh};
    const int starts[4] = {0, K * t, K * t + t, K * t + 2 * t};
    return recalgo_slabs::launch_colsums(ws, rows, 3, outs, starts, st);
}
