// DCN-V2's cross layer, the mixture of low-rank experts (include/recalgo_dcnv2.h; Wang et al., WWW 2021, eq. 4).
//
// A workgroup of four waves takes a tile of 16 examples as the M of v_mfma_f32_16x16x4_f32: lane l = (r16, q) = (l & 15, l >> 4)
// supplies A[m = r16][k = q] and B[k = q][n = r16] of a k-step and receives C[m = 4 q + i][n = r16] in register i.  The A
// operands (the xl tile, q = g * x0, v, c, ..) are read from LDS, where a row is padded with zeros to the tile width; the weights
// are B operands read through L2 (E 2 D r floats do not fit LDS), an index past the end clamped to the last valid one: its A
// partner is a zero of the padding, or the column it yields is not stored.  The phases of a tile are split over the waves by
// (expert, 16-column tile of r) and by 16-column tile of D, with a barrier between two phases:
//
//   forward   v = tanh(xl V_e), s = xl gate^T  |  p = softmax(s)  |  pc = p_e tanh(v C_e)  |  y = x0 * (pc U^T + bias) + xl
//             (the last product runs over the E r columns of all experts at once: the mixture is ONE chain per column tile of D)
//   backward  v, s, t_e = q U_e  |  c  |  dp_e = c_e . t_e, p, ds (wave 0)  |  dcpre = p_e t_e (1 - c^2)  |
//             dvpre = (dcpre C_e^T)(1 - v^2)  |  dx0 = g * (pc U^T + bias), dxl = g + dvpre V^T + ds gate
//             (dp_e leaves out q . bias: it is the same for every expert and cancels in ds_e = p_e (dp_e - sum p dp))
//
// An output row's k-order is the same in every row of a tile, so an example's y, dx0 and dxl do not depend on its place.
//
// Weight gradients: the E 2 D r accumulators do not fit a workgroup's registers, so the backward kernel leaves pc, dvpre, v, dcpre
// and ds per example in the workspace ([B, E r]-sized) and dcnv2_wgrad_kernel forms the partial rows from them: a wave per
// (row, 16-row tile of one gradient), the examples of the row as the K of the MFMAs, in example order.  dbias and dgate ride on
// the tiles of expert 0.  recalgo_slabs::launch_colsums sums the rows.
#include "common.h"
#include "slab_sum.h"
#include "../../include/recalgo_dcnv2.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;
constexpr int kTile = RECALGO_DCNV2_TILE;
constexpr int kMaxE = RECALGO_DCNV2_MAX_E;
constexpr int kGrid = 1024;                                  // workgroups of the tile kernels; they loop over their tiles
constexpr int kMaxRT = RECALGO_DCNV2_MAX_R / 16;

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

struct CxArgs {
    const float *x0, *xl, *V, *C, *U, *gate, *bias;
    int B, D, r, E;
};

// The LDS layout, in floats: rows of 16 examples.  ldx = 4 (mod 16) and ldc = 4 (mod 16) keep the 16 rows x 4 k of an A operand
// on 64 different banks.
struct CxLds {
    int ldx, ldc;
    int XL, Q, VS, CS, T, DV, S, P, DP, DS;                 // (forward: XL, VS, CS (= pc), S, P)
    int total;
};

int round16(int v) { return (v + 15) & ~15; }

CxLds cx_lds(int D, int r, int E, bool bwd) {
    CxLds L;
    L.ldx = round16(D) + 4, L.ldc = round16(E * r) + 4;
    int n = 0;
    L.XL = n, n += kTile * L.ldx;
    L.Q = n, n += bwd ? kTile * L.ldx : 0;
    L.VS = n, n += kTile * L.ldc;
    L.CS = n, n += kTile * L.ldc;
    L.T = n, n += bwd ? kTile * L.ldc : 0;
    L.DV = n, n += bwd ? kTile * L.ldc : 0;
    L.S = n, n += kTile * kMaxE;
    L.P = n, n += kTile * kMaxE;
    L.DP = n, n += bwd ? kTile * kMaxE : 0;
    L.DS = n, n += bwd ? kTile * kMaxE : 0;
    L.total = n;
    return L;
}

bool shape_ok(int D, int r, int E) {
    return D >= RECALGO_DCNV2_MIN_D && D <= RECALGO_DCNV2_MAX_D && r >= RECALGO_DCNV2_MIN_R && r <= RECALGO_DCNV2_MAX_R &&
           (r & 3) == 0 && E >= 1 && E <= RECALGO_DCNV2_MAX_E;
}

int partial_rows(int B) {
    const int rows = cdiv(cdiv(B, kTile), RECALGO_DCNV2_ROW_TILES);
    return rows > RECALGO_DCNV2_MAX_PARTIAL_ROWS ? RECALGO_DCNV2_MAX_PARTIAL_ROWS : rows;
}

int64_t row_floats(int D, int r, int E, bool gated) { return (int64_t)E * (2 * D * r + r * r + (gated ? D : 0)) + D; }

// ---- device ---------------------------------------------------------------------------------------------------------------------
// acc + sum over n k-steps of (as * A[4 s]) * Bp[min(4 s + q, K - 1) * bs]: `A` carries the lane's LDS row and k = q, `Bp` its
// column.  Four partial sums, k-step s into partial s % 4 (the tail into partial 0), added pairwise at the end: a quarter of the
// chain's rounding growth, four independent MFMA chains in flight, and eight loads issued before the first of them is needed.
__device__ __forceinline__ f32x4 mm_g(const float* A, const float* __restrict__ Bp, int bs, int K, int n, int q, f32x4 acc,
                                      float as = 1.f) {
    f32x4 p0 = zero4(), p1 = zero4(), p2 = zero4(), p3 = zero4();
    int s = 0;
    for (; s + 8 <= n; s += 8) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = 4 * (s + u) + q;
            av[u] = as * A[4 * (s + u)], bv[u] = Bp[(size_t)(k < K ? k : K - 1) * bs];
        }
        p0 = mfma16(av[0], bv[0], p0), p1 = mfma16(av[1], bv[1], p1), p2 = mfma16(av[2], bv[2], p2), p3 = mfma16(av[3], bv[3], p3);
        p0 = mfma16(av[4], bv[4], p0), p1 = mfma16(av[5], bv[5], p1), p2 = mfma16(av[6], bv[6], p2), p3 = mfma16(av[7], bv[7], p3);
    }
    if (s + 4 <= n) {
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = 4 * (s + u) + q;
            av[u] = as * A[4 * (s + u)], bv[u] = Bp[(size_t)(k < K ? k : K - 1) * bs];
        }
        p0 = mfma16(av[0], bv[0], p0), p1 = mfma16(av[1], bv[1], p1), p2 = mfma16(av[2], bv[2], p2), p3 = mfma16(av[3], bv[3], p3);
        s += 4;
    }
    for (; s < n; ++s) {
        const int k = 4 * s + q;
        p0 = mfma16(as * A[4 * s], Bp[(size_t)(k < K ? k : K - 1) * bs], p0);
    }
    return acc + ((p0 + p1) + (p2 + p3));
}

// dst [16][ldx] <- rows b0 .. b0 + 15 of src [B, D] (times mul's, where given), zeros past B and past D
__device__ __forceinline__ void stage_rows(float* dst, int ldx, const float* __restrict__ src, const float* __restrict__ mul,
                                           long long b0, int B, int D) {
    for (int idx = threadIdx.x; idx < kTile * ldx; idx += 64 * kWaves) {
        const int m = idx / ldx, c = idx - m * ldx;
        const long long b = b0 + m;
        float v = 0.f;
        if (b < B && c < D) {
            v = src[(size_t)b * D + c];
            if (mul != nullptr) v *= mul[(size_t)b * D + c];
        }
        dst[idx] = v;
    }
}

// the phase both ways share: VS = tanh(xl V_e), S = xl gate^T and (backward, Qs given) T_e = q U_e, split over the waves
__device__ __forceinline__ void project(const CxArgs& a, const CxLds& L, float* sm, const float* Qs, int wave, int r16, int q) {
    const int RT = (a.r + 15) >> 4, kD = (a.D + 3) >> 2, nV = a.E * RT, nT = Qs != nullptr ? nV : 0;
    for (int it = wave; it < nV + nT + 1; it += kWaves) {
        if (it < nV + nT) {
            const bool second = it >= nV;
            const int e = (second ? it - nV : it) / RT, jt = (second ? it - nV : it) % RT;
            const int j = 16 * jt + r16, jc = j < a.r ? j : a.r - 1;
            const float* W = (second ? a.U : a.V) + (size_t)e * a.D * a.r + jc;
            const f32x4 acc = mm_g((second ? Qs : sm + L.XL) + r16 * L.ldx + q, W, a.r, a.D, kD, q, zero4());
            float* dst = sm + (second ? L.T : L.VS);
            if (j < a.r) {
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[(4 * q + i) * L.ldc + e * a.r + j] = second ? acc[i] : tanhf(acc[i]);
            }
        } else if (a.gate != nullptr) {
            const int ec = r16 < a.E ? r16 : a.E - 1;
            const f32x4 acc = mm_g(sm + L.XL + r16 * L.ldx + q, a.gate + (size_t)ec * a.D, 1, a.D, kD, q, zero4());
            if (r16 < a.E) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sm[L.S + (4 * q + i) * kMaxE + r16] = acc[i];
            }
        }
    }
}

// CS = tanh(v C_e), times p_e where `scaled` (the forward keeps p_e c_e alone)
__device__ __forceinline__ void project_c(const CxArgs& a, const CxLds& L, float* sm, bool scaled, int wave, int r16, int q) {
    const int RT = (a.r + 15) >> 4;
    for (int it = wave; it < a.E * RT; it += kWaves) {
        const int e = it / RT, jt = it % RT, j = 16 * jt + r16, jc = j < a.r ? j : a.r - 1;
        const f32x4 acc = mm_g(sm + L.VS + r16 * L.ldc + e * a.r + q, a.C + (size_t)e * a.r * a.r + jc, a.r, a.r, a.r >> 2, q, zero4());
        if (j < a.r) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float c = tanhf(acc[i]);
                sm[L.CS + (4 * q + i) * L.ldc + e * a.r + j] = scaled ? sm[L.P + (4 * q + i) * kMaxE + e] * c : c;
            }
        }
    }
}

// row m's softmax over the experts, shifted by its maximum (without a gate: E == 1 and p = 1)
__device__ __forceinline__ void softmax_row(const CxArgs& a, const float* S, float (&p)[kMaxE]) {
    float mx = -INFINITY, sum = 0.f;
#pragma unroll
    for (int e = 0; e < kMaxE; ++e)
        if (e < a.E) mx = fmaxf(mx, S[e]);
#pragma unroll
    for (int e = 0; e < kMaxE; ++e) {
        p[e] = e < a.E ? expf(S[e] - mx) : 0.f;
        sum += p[e];
    }
#pragma unroll
    for (int e = 0; e < kMaxE; ++e) p[e] = a.gate != nullptr ? p[e] / sum : (e == 0 ? 1.f : 0.f);
}

__global__ __launch_bounds__(64 * kWaves) void dcnv2_fwd_kernel(CxArgs a, CxLds L, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int tiles = (a.B + kTile - 1) / kTile, DT = (a.D + 15) >> 4, kR = a.r >> 2;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long b0 = (long long)t * kTile;
        stage_rows(sm + L.XL, L.ldx, a.xl, nullptr, b0, a.B, a.D);
        __syncthreads();
        project(a, L, sm, nullptr, wave, r16, q);
        __syncthreads();
        if (threadIdx.x < kTile) {
            float p[kMaxE];
            softmax_row(a, sm + L.S + threadIdx.x * kMaxE, p);
#pragma unroll
            for (int e = 0; e < kMaxE; ++e) sm[L.P + threadIdx.x * kMaxE + e] = p[e];
        }
        __syncthreads();
        project_c(a, L, sm, true, wave, r16, q);
        __syncthreads();
        for (int nt = wave; nt < DT; nt += kWaves) {
            const int n = 16 * nt + r16, nc = n < a.D ? n : a.D - 1;
            f32x4 acc = zero4();
            for (int e = 0; e < a.E; ++e)
                acc = mm_g(sm + L.CS + r16 * L.ldc + e * a.r + q, a.U + ((size_t)e * a.D + nc) * a.r, 1, a.r, kR, q, acc);
            const float bn = a.bias[nc];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long b = b0 + 4 * q + i;
                if (b < a.B && n < a.D)
                    y[(size_t)b * a.D + n] = fmaf(a.x0[(size_t)b * a.D + n], acc[i] + bn, sm[L.XL + (4 * q + i) * L.ldx + n]);
            }
        }
        __syncthreads();                                     // (the next tile overwrites XL)
    }
}

// the per-example part of the workspace (recalgo_dcnv2.h)
struct CxSaved {
    float *pc, *dv, *v, *dc, *ds;
};

__global__ __launch_bounds__(64 * kWaves) void dcnv2_bwd_kernel(CxArgs a, CxLds L, const float* __restrict__ g,
                                                                float* __restrict__ dx0, float* __restrict__ dxl, CxSaved w) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int tiles = (a.B + kTile - 1) / kTile, DT = (a.D + 15) >> 4, RT = (a.r + 15) >> 4, kR = a.r >> 2, ER = a.E * a.r;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long b0 = (long long)t * kTile;
        stage_rows(sm + L.XL, L.ldx, a.xl, nullptr, b0, a.B, a.D);
        stage_rows(sm + L.Q, L.ldx, g, a.x0, b0, a.B, a.D);
        __syncthreads();
        project(a, L, sm, sm + L.Q, wave, r16, q);
        __syncthreads();
        project_c(a, L, sm, false, wave, r16, q);
        __syncthreads();
        if (wave == 0) {
            // dp_e = c_e . t_e by lane (m = r16, e = q), then a lane per row: p, ds
            if (q < a.E) {
                const float *c = sm + L.CS + r16 * L.ldc + q * a.r, *tt = sm + L.T + r16 * L.ldc + q * a.r;
                float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;         // (four partial sums over k % 4, added pairwise)
                for (int k = 0; k < a.r; k += 4)
                    d0 = fmaf(c[k], tt[k], d0), d1 = fmaf(c[k + 1], tt[k + 1], d1), d2 = fmaf(c[k + 2], tt[k + 2], d2),
                    d3 = fmaf(c[k + 3], tt[k + 3], d3);
                sm[L.DP + r16 * kMaxE + q] = (d0 + d1) + (d2 + d3);
            }
            wave_sync();
            if (lane < kTile) {
                float p[kMaxE], dot = 0.f;
                softmax_row(a, sm + L.S + lane * kMaxE, p);
#pragma unroll
                for (int e = 0; e < kMaxE; ++e)
                    if (e < a.E) dot = fmaf(p[e], sm[L.DP + lane * kMaxE + e], dot);
#pragma unroll
                for (int e = 0; e < kMaxE; ++e) {
                    const float ds = e < a.E ? p[e] * (sm[L.DP + lane * kMaxE + e] - dot) : 0.f;
                    sm[L.P + lane * kMaxE + e] = p[e], sm[L.DS + lane * kMaxE + e] = ds;
                    if (b0 + lane < a.B) w.ds[(size_t)(b0 + lane) * kMaxE + e] = ds;
                }
            }
        }
        __syncthreads();
        // dcpre = p_e t_e (1 - c^2) takes the place of t; pc, v and dcpre go to the workspace
        for (int idx = threadIdx.x; idx < kTile * ER; idx += 64 * kWaves) {
            const int m = idx / ER, col = idx - m * ER, e = col / a.r;
            const float c = sm[L.CS + m * L.ldc + col], p = sm[L.P + m * kMaxE + e];
            const float dc = p * sm[L.T + m * L.ldc + col] * fmaf(-c, c, 1.f);
            sm[L.T + m * L.ldc + col] = dc;
            if (b0 + m < a.B) {
                const size_t o = (size_t)(b0 + m) * ER + col;
                w.pc[o] = p * c, w.dc[o] = dc, w.v[o] = sm[L.VS + m * L.ldc + col];
            }
        }
        __syncthreads();
        // dvpre_e = (dcpre_e C_e^T) (1 - v_e^2)
        for (int it = wave; it < a.E * RT; it += kWaves) {
            const int e = it / RT, jt = it % RT, j = 16 * jt + r16, jc = j < a.r ? j : a.r - 1;
            const f32x4 acc = mm_g(sm + L.T + r16 * L.ldc + e * a.r + q, a.C + ((size_t)e * a.r + jc) * a.r, 1, a.r, kR, q, zero4());
            if (j < a.r) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = 4 * q + i;
                    const float v = sm[L.VS + m * L.ldc + e * a.r + j], dv = acc[i] * fmaf(-v, v, 1.f);
                    sm[L.DV + m * L.ldc + e * a.r + j] = dv;
                    if (b0 + m < a.B) w.dv[(size_t)(b0 + m) * ER + e * a.r + j] = dv;
                }
            }
        }
        __syncthreads();
        for (int nt = wave; nt < DT; nt += kWaves) {
            const int n = 16 * nt + r16, nc = n < a.D ? n : a.D - 1;
            f32x4 am = zero4(), ax = zero4();
            for (int e = 0; e < a.E; ++e) {
                am = mm_g(sm + L.CS + r16 * L.ldc + e * a.r + q, a.U + ((size_t)e * a.D + nc) * a.r, 1, a.r, kR, q, am,
                          sm[L.P + r16 * kMaxE + e]);
                ax = mm_g(sm + L.DV + r16 * L.ldc + e * a.r + q, a.V + ((size_t)e * a.D + nc) * a.r, 1, a.r, kR, q, ax);
            }
            if (a.gate != nullptr)                           // + sum_e ds_e gate_e: one k-step over the (padded) experts
                ax = mfma16(sm[L.DS + r16 * kMaxE + q], q < a.E ? a.gate[(size_t)q * a.D + nc] : 0.f, ax);
            const float bn = a.bias[nc];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long b = b0 + 4 * q + i;
                if (b < a.B && n < a.D) {
                    const float gg = g[(size_t)b * a.D + n];
                    dx0[(size_t)b * a.D + n] = gg * (am[i] + bn);
                    dxl[(size_t)b * a.D + n] = gg + ax[i];
                }
            }
        }
        __syncthreads();                                     // (the next tile overwrites every buffer)
    }
}

// One wave per (partial row, item).  Items: dU_e and dV_e by 16-row tile of D, dC_e by 16-row tile of r; each is
// sum over the row's examples of a^T b with a = q | xl | v_e (the MFMA's M) and b = pc_e | dvpre_e | dcpre_e (its N, all r
// columns in RT accumulators).  The dU tiles of expert 0 carry dbias = sum q as one more column, the dV tiles dgate = xl^T ds.
__global__ __launch_bounds__(64) void dcnv2_wgrad_kernel(CxArgs a, const float* __restrict__ g, CxSaved w, float* __restrict__ rows,
                                                         int n_rows, int row_len) {
    const int lane = threadIdx.x, r16 = lane & 15, q = lane >> 4;
    const int DT = (a.D + 15) >> 4, RT = (a.r + 15) >> 4, ER = a.E * a.r, nDU = a.E * DT;
    const int tiles = (a.B + kTile - 1) / kTile, s = blockIdx.y;
    const long long b_lo = (long long)kTile * (int)((long long)s * tiles / n_rows);
    long long b_hi = (long long)kTile * (int)((long long)(s + 1) * tiles / n_rows);
    if (b_hi > a.B) b_hi = a.B;
    const int item = blockIdx.x;
    const int kind = item < nDU ? 0 : (item < 2 * nDU ? 1 : 2);              // dU, dV, dC
    const int local = item - kind * nDU, e = kind < 2 ? local / DT : local / RT, mt = kind < 2 ? local % DT : local % RT;
    const int M = kind < 2 ? a.D : a.r, mrow = 16 * mt + r16, mc = mrow < M ? mrow : M - 1;
    const float* bsrc = (kind == 0 ? w.pc : (kind == 1 ? w.dv : w.dc)) + e * a.r;
    const bool extra = kind < 2 && e == 0 && (kind == 0 || a.gate != nullptr);

    f32x4 acc[kMaxRT], odd[kMaxRT], ex = zero4();           // (even and odd k-steps apart: half the chain's rounding growth)
#pragma unroll
    for (int jt = 0; jt < kMaxRT; ++jt) acc[jt] = zero4(), odd[jt] = zero4();
    constexpr int kU = 4;                                    // k-steps whose loads are in flight together
    for (long long bb = b_lo; bb < b_hi; bb += 4 * kU) {
        float av[kU], bv[kU][kMaxRT], xv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long bq = bb + 4 * u + q;
            const bool live = bq < b_hi && mrow < M;
            const size_t b = bq < b_hi ? bq : b_hi - 1;
            float v;
            if (kind == 0) v = g[b * a.D + mc] * a.x0[b * a.D + mc];
            else if (kind == 1) v = a.xl[b * a.D + mc];
            else v = w.v[b * ER + e * a.r + mc];
            av[u] = live ? v : 0.f;
#pragma unroll
            for (int jt = 0; jt < kMaxRT; ++jt) {
                const int j = 16 * jt + r16;
                bv[u][jt] = jt < RT ? bsrc[b * ER + (j < a.r ? j : a.r - 1)] : 0.f;
            }
            xv[u] = !extra ? 0.f : (kind == 0 ? (r16 == 0 ? 1.f : 0.f) : (r16 < a.E ? w.ds[b * kMaxE + r16] : 0.f));
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {                       // (a step past the row's end adds zeros: av = 0)
#pragma unroll
            for (int jt = 0; jt < kMaxRT; ++jt)
                if (jt < RT) {
                    if (u & 1) odd[jt] = mfma16(av[u], bv[u][jt], odd[jt]);
                    else acc[jt] = mfma16(av[u], bv[u][jt], acc[jt]);
                }
            if (extra) ex = mfma16(av[u], xv[u], ex);
        }
    }

    const bool gated = a.gate != nullptr;
    const size_t DR = (size_t)a.D * a.r, RR = (size_t)a.r * a.r;
    const size_t oV = 0, oC = a.E * DR, oU = oC + a.E * RR, oG = oU + a.E * DR, oB = oG + (gated ? (size_t)a.E * a.D : 0);
    float* row = rows + (size_t)s * row_len;
    float* dst = row + (kind == 0 ? oU + e * DR : (kind == 1 ? oV + e * DR : oC + e * RR));
#pragma unroll
    for (int jt = 0; jt < kMaxRT; ++jt)
        if (jt < RT) {
            const int j = 16 * jt + r16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mm = 16 * mt + 4 * q + i;
                if (mm < M && j < a.r) dst[(size_t)mm * a.r + j] = acc[jt][i] + odd[jt][i];
            }
        }
    if (extra) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = 16 * mt + 4 * q + i;
            if (d < a.D && kind == 0 && r16 == 0) row[oB + d] = ex[i];
            if (d < a.D && kind == 1 && r16 < a.E) row[oG + (size_t)r16 * a.D + d] = ex[i];
        }
    }
}

}  // namespace

RECALGO_EXPORT int recalgo_dcnv2_abi_version(void) { return RECALGO_DCNV2_ABI_VERSION; }

RECALGO_EXPORT int recalgo_dcnv2_supported(int D, int r, int E) { return shape_ok(D, r, E) ? 1 : 0; }

RECALGO_EXPORT int recalgo_dcnv2_bwd_partial_rows(int B, int D, int r, int E) {
    if (B < 1 || !shape_ok(D, r, E)) return 0;
    return partial_rows(B);
}

RECALGO_EXPORT int64_t recalgo_dcnv2_bwd_workspace_bytes(int B, int D, int r, int E) {
    if (B < 1 || !shape_ok(D, r, E)) return 0;
    return (int64_t)sizeof(float) * (partial_rows(B) * row_floats(D, r, E, true) + (int64_t)B * (4 * E * r + kMaxE));
}

RECALGO_EXPORT int recalgo_dcnv2_layer_fwd(const float* x0, const float* xl, const float* V, const float* C, const float* U,
                                           const float* gate, const float* bias, int B, int D, int r, int E, float* y,
                                           recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(D, r, E));
    RECALGO_REQUIRE(x0 && xl && V && C && U && bias && y);
    RECALGO_REQUIRE(gate != nullptr || E == 1);
    RECALGO_REQUIRE(aligned_to<4>(x0, xl, V, C, U, gate, bias, y));
    const CxLds L = cx_lds(D, r, E, false);
    const CxArgs a = {x0, xl, V, C, U, gate, bias, B, D, r, E};
    const int tiles = cdiv(B, kTile);
    RECALGO_CHECK(launch_lds<dcnv2_fwd_kernel>(dim3(tiles < kGrid ? tiles : kGrid), dim3(64 * kWaves), sizeof(float) * (size_t)L.total,
                                               as_stream(stream), a, L, y));
    RECALGO_RETURN_LAST();
}

RECALGO_EXPORT int recalgo_dcnv2_layer_bwd(const float* g, const float* x0, const float* xl, const float* V, const float* C,
                                           const float* U, const float* gate, const float* bias, int B, int D, int r, int E,
                                           float* dx0, float* dxl, float* dV, float* dC, float* dU, float* dgate, float* dbias,
                                           void* workspace, recalgo_stream_t stream) {
    RECALGO_REQUIRE(B >= 1 && shape_ok(D, r, E));
    RECALGO_REQUIRE(g && x0 && xl && V && C && U && bias && dx0 && dxl && dV && dC && dU && dbias && workspace);
    RECALGO_REQUIRE((gate == nullptr) == (dgate == nullptr));
    RECALGO_REQUIRE(gate != nullptr || E == 1);
    RECALGO_REQUIRE(aligned_to<4>(g, x0, xl, V, C, U, gate, bias, dx0, dxl, dV, dC, dU, dgate, dbias) && aligned_to<4>(workspace));
    const bool gated = gate != nullptr;
    const CxLds L = cx_lds(D, r, E, true);
    const CxArgs a = {x0, xl, V, C, U, gate, bias, B, D, r, E};
    const int tiles = cdiv(B, kTile), rows = partial_rows(B), row_len = (int)row_floats(D, r, E, gated);
    hipStream_t st = as_stream(stream);
    float* ws = static_cast<float*>(workspace);
    const size_t per = (size_t)B * E * r;
    float* saved = ws + (size_t)rows * row_floats(D, r, E, true);
    const CxSaved w = {saved, saved + per, saved + 2 * per, saved + 3 * per, saved + 4 * per};
    RECALGO_CHECK(launch_lds<dcnv2_bwd_kernel>(dim3(tiles < kGrid ? tiles : kGrid), dim3(64 * kWaves), sizeof(float) * (size_t)L.total,
                                               st, a, L, g, dx0, dxl, w));
    const int DT = cdiv(D, 16), RT = cdiv(r, 16);
    hipLaunchKernelGGL(dcnv2_wgrad_kernel, dim3(E * (2 * DT + RT), rows), dim3(64), 0, st, a, g, w, ws, rows, row_len);
    const int DR = D * r, RR = r * r;
    float* const outs[5] = {dV, dC, dU, gated ? dgate : dbias, dbias};
    const int starts[6] = {0, E * DR, E * (DR + RR), E * (2 * DR + RR), row_len - (gated ? D : 0), row_len};
    if (!gated) {
        const int starts4[5] = {0, E * DR, E * (DR + RR), E * (2 * DR + RR), row_len};
        return recalgo_slabs::launch_colsums(ws, rows, 4, outs, starts4, st);
    }
    return recalgo_slabs::launch_colsums(ws, rows, 5, outs, starts, st);
}
